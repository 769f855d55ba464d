"""What the rollout (npb_set_rollout: trajectories recorded on the device, GAE advantages in one launch) costs on BASELINE config 4 at
65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5) with device noise and autoreset (max_episode_steps 64, so plants truncate inside the horizon):
no per-step host input.  Features of 16 columns x 4 frames, float32; controls of 4 axes (rod RATE, valve RATE, flow RATE, a VALUE axis),
float32 input, one fixed [n, 4] tensor whose sign is flipped in place before every step in EVERY setup; E = 2 extras; T = 128.  A block is
one horizon: T steps, then the rewind.  One handle per size throughout; the rollout is set and dropped on it between blocks, in an order
that rotates from round to round.  Setups, event-timed us per step:
  off      features and controls on, no rollout                                                                                  (a)
  on       the rollout on: the pre and the post kernel around every step                                                         (b)
  torch    no rollout; the same recording the way a user does it today on the same build: buf[t].copy_(...) for the features, the
           controls input, the extras, the reward, done and the truncated column -- six launches -- and for the truncated plants'
           terminal stacks a nonzero() of the truncated column (a host synchronisation) and an index_select of final_features()        (b)
and, on the recorded rollout, us per call:
  advantages        rollout_advantages(0.99, 0.95) with values from the extras in place, float32 outputs                          (c)
  advantages_torch  the same recurrence as a torch loop over T on the same tensors, float64, selects for the bootstrap and the carry  (c)
Reported per setup: the per-step time of each block (median, quartiles, min..max over the blocks), each setup minus off of the same round,
and whether the device path is below the by-hand one -- as measured, whichever way it falls.

--parent DIR: a checkout of the parent commit, built.  `off` is then also measured in fresh processes, alternately on this build and on
the parent's (this script run with --package-root and --only-off), `--process-repeats` times each, and held against each other by
overhead_harness.compare_off.  One JSON line per run, all sizes in one object, also written to --out.
"""
import argparse
import os
import sys

import numpy as np

from overhead_harness import add_parent_arguments, compare_off, head, off_across_builds, paired, rotated_blocks, stats, time_steps, write_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 8
DT = 5.0
T, E, K, C, L = 128, 2, 4, 16, 64
AXES = [("rod", "rate"), ("valve", "rate"), ("flow", "rate"), (None, "value")]
GAMMA, LAM = 0.99, 0.95


def columns():
    from nuclear_sim_amd.env import INFO_COLUMNS
    return ([("obs", i) for i in range(8)] + [("info", name) for name in INFO_COLUMNS[:4]] +
            ["reward", ("pump.oil_level", 0), ("pump.oil_level", 1), "prim.fuel_temperature"])[:C]


class ByHand:
    """the same record with what the package offers without set_rollout"""

    def __init__(self, env, extras):
        import torch
        self.torch, self.env, self.extras = torch, env, extras
        n, dev = env.n, env.device
        f = env.features()
        self.obs = torch.zeros((T,) + tuple(f.shape), dtype=f.dtype, device=dev)
        self.act = torch.zeros((T, n, len(AXES)), dtype=torch.float32, device=dev)
        self.extra = torch.zeros((T, n, E), dtype=torch.float32, device=dev)
        self.reward = torch.zeros((T, n), dtype=torch.float64, device=dev)
        self.done = torch.zeros((T, n), dtype=torch.uint8, device=dev)
        self.truncated = torch.zeros((T, n), dtype=torch.uint8, device=dev)
        self.begin()

    def begin(self):
        self.t, self.finals = 0, []

    def step(self, x):
        env, t = self.env, self.t
        self.obs[t].copy_(env.features())
        self.act[t].copy_(x)
        self.extra[t].copy_(self.extras)
        obs, rew, done, info = env.step()
        self.reward[t].copy_(rew)
        self.done[t].copy_(done)
        self.truncated[t].copy_(info["truncated"])
        idx = self.torch.nonzero(info["truncated"]).squeeze(1)      # (the host waits here)
        if idx.numel():
            self.finals.append((t, idx, info["final_features"].index_select(0, idx)))
        self.t = t + 1


def advantages_in_torch(torch, reward, ended, final_row, value, last_value, final_value, gamma, lam):
    """the statement's recurrence as a torch loop over the slots: float64, selects for the bootstrap and the carry"""
    Tn, n = reward.shape
    adv, ret = torch.empty_like(reward), torch.empty_like(reward)
    gl = gamma * lam
    zero = torch.zeros(n, dtype=torch.float64, device=reward.device)
    a_next, v_next = zero, last_value.to(torch.float64)
    for t in range(Tn - 1, -1, -1):
        e, v = ended[t], value[t].to(torch.float64)
        fin = torch.where(final_row[t] >= 0, final_value[final_row[t].clamp(min=0).long()].to(torch.float64), zero)
        nv = torch.where((e & 5) != 0, zero, torch.where((e & 2) != 0, fin, v_next))
        a = ((reward[t] + gamma * nv) - v) + gl * torch.where((e & 7) != 0, zero, a_next)
        adv[t], ret[t] = a, a + v
        a_next, v_next = a, v
    return adv.to(torch.float32), ret.to(torch.float32)


def measure(n, rounds, only_off, calls):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, noise_generator="device", autoreset=True, max_episode_steps=L)
    env.set_features(columns(), stack=K, final=True)
    env.set_controls(AXES)
    has = hasattr(env, "set_rollout") and not only_off
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    env.controls_input().copy_(((torch.rand((n, len(AXES)), generator=g) * 2.0 - 1.0) * 0.02).to(torch.float32))
    x = env.controls_input()
    extras = (torch.rand((n, E), generator=g) - 0.5).to(device=dev, dtype=torch.float32)
    setups = ["off"] + (["on", "torch"] if has else [])
    env.features()
    by_hand = ByHand(env, extras) if has else None

    def step(setup):
        x.neg_()      # the policy's new output, in every setup
        if setup == "torch":
            return by_hand.step(x)
        return env.step()

    def run_block(setup):
        if has:
            if setup == "on":
                if env._roll is None:
                    env.set_rollout(T, extras=E)
                    env.rollout_extras_input().copy_(extras)
                env.rollout_begin()
                for _ in range(W):
                    step(setup)
                env.rollout_begin()
            else:
                env.set_rollout(None)
                for _ in range(W):
                    step("off")
                by_hand.begin()
        else:
            for _ in range(W):
                step(setup)
        return time_steps(stream, lambda: step(setup), T)

    blocks = rotated_blocks(setups, rounds, run_block)
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": T, "rounds": rounds,
           "features": [K, C], "axes": len(AXES), "extras": E, "max_episode_steps": L, "setups": {s: stats(v) for s, v in blocks.items()}}
    if has:
        out["on_cost_us_per_step"] = paired(blocks, "on", "off")
        out["by_hand_in_torch_cost_us_per_step"] = paired(blocks, "torch", "off")
        out["on_percent_of_the_step"] = 100.0 * out["on_cost_us_per_step"]["median"] / out["setups"]["off"]["median_us"]
        out["on_is_below_by_hand"] = bool(out["on_cost_us_per_step"]["median"] < out["by_hand_in_torch_cost_us_per_step"]["median"])
        # (c): a full horizon recorded, then the advantages on the device and as a torch loop over the same tensors
        env.set_rollout(T, extras=E)
        env.rollout_extras_input().copy_(extras)
        for _ in range(T):
            step("on")
        r = env.rollout()
        R = env.rollout_spec()["final_rows"]
        last = (torch.rand(n, generator=g) - 0.5).to(device=dev, dtype=torch.float32)
        final = (torch.rand(n * R, generator=g) - 0.5).to(device=dev, dtype=torch.float32)
        value = r["extra"][:, :, 0].contiguous()

        def call(which):
            if which == "advantages":
                return env.rollout_advantages(GAMMA, LAM, values=("extra", 0), last_value=last, final_values=final)
            return advantages_in_torch(torch, r["reward"], r["ended"], r["final_row"], value, last, final, GAMMA, LAM)
        times, res = {"advantages": [], "advantages_torch": []}, {}

        def keep(which):
            res[which] = call(which)
        for which in times:
            us = [time_steps(stream, lambda: keep(which), 1) for _ in range(W // 2 + calls)]
            times[which] = (us[W // 2:], [t.clone() for t in res[which]])
        same = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(times["advantages"][1], times["advantages_torch"][1]))
        out["advantages"] = {"slots": T, "truncated_transitions": int((r["ended"] == 2).sum().item()), "device": stats(times["advantages"][0]),
                             "torch_loop": stats(times["advantages_torch"][0]), "the_two_agree_by_bits": bool(same),
                             "device_is_below_the_loop": bool(np.median(times["advantages"][0]) < np.median(times["advantages_torch"][0]))}
        env.set_rollout(None)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="timed calls of each advantages path")
    add_parent_arguments(ap, "rollout_overhead.json")
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    sizes = {}
    for n in a.n:
        res = measure(n, a.rounds, a.only_off, a.calls)
        print("%d plants: measured" % n, file=sys.stderr, flush=True)
        if a.parent and not a.only_off:
            this, parent = off_across_builds(__file__, ["--n", n, "--rounds", a.rounds], a.parent, a.process_repeats,
                                             lambda run: run["sizes"][str(n)]["setups"]["off"]["median_us"], 900)
            res["parent_comparison"] = {"off": compare_off(this, parent, res["setups"]["off"])}
        sizes[str(n)] = res
    out = {"what": "per-step time of config 4 with device noise and autoreset (max_episode_steps 64), features of 16 columns x 4 frames float32, "
                   "controls of 4 axes: the rollout (T = 128, E = 2) off and on; the same recording done by hand in torch on the same build "
                   "beside it; and rollout_advantages against the same recurrence as a torch loop over T",
           "sizes": sizes, "head": head(ROOT)}
    write_line(out, a.out)


if __name__ == "__main__":
    main()
