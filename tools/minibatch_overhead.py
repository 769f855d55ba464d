"""What the shuffled minibatches and the pinned moments (npb_rollout_minibatch, npb_rollout_moments) cost over a recorded rollout of the
README's shape, at 65 536 and 32 768 plants, beside the same work done by hand in torch on the same tensors.

action_test("oil_top_off", range(n), dt = 5) with device noise and autoreset (max_episode_steps 64); features of 16 columns x 4 frames
float32, controls of 4 axes, E = 2 extras, T = 128.  One full horizon is recorded and rollout_advantages(0.99, 0.95) forms float32
advantages; on that rollout, event-timed on the env's stream, an EPOCH (one pass over all T * n transitions) by each of
  device      env.rollout_minibatches(65 536, normalize=True): the moments once (four launches), then one launch per minibatch
  plant       the same with unit="plant", 65 536 / T = 512 plants a minibatch, sequences whole, [T, 512, ...]
  by_hand_a   what a user does today: adv.mean() / adv.std() once, torch.randperm(T * n) per epoch, and per minibatch a slice of the permutation, five
  by_hand_b   index_selects (obs, act, extra, adv, ret) and (adv - mean) / (std + 1e-8); run as two setups of their own, so that their
              difference is the comparison's own noise
in an order that rotates from round to round, REPS epochs in every timed window (moments, mean and std once per window); and
env.rollout_moments() alone, us per call.  Per setup: the epoch's time (median,
quartiles, min..max over the rounds), per-minibatch time = epoch / minibatches (the device's includes its share of the moments), and the
achieved bytes/s of a device minibatch: the bytes gathered plus the bytes written (each gathered row once in, once out, and the index),
over the per-minibatch time, beside the 8 TB/s the project prices against.  The claim `device_epoch_is_below_by_hand`: the by-hand epoch
(the lower of the two medians) minus the device's exceeds the spread of the two by-hand medians -- as measured, whichever way it falls.
Torch's normalised advantages differ from the device's in the last bits, its reduction being its own: the largest difference is reported,
and so is that of the moments themselves; the indices necessarily differ.

`off`: the step with features, controls and the rollout on, nothing of this feature called -- what the parent commit's build runs too.
--parent DIR: a checkout of the parent commit, built.  `off` is then measured in fresh processes, alternately on this build and on the
parent's (this script run with --package-root and --only-off), `--process-repeats` times each, and held against each other by
overhead_harness.compare_off.  One JSON line per run, all sizes in one object, also written to --out.
"""
import argparse
import os
import sys

from overhead_harness import add_parent_arguments, compare_off, head, off_across_builds, stats, time_steps, write_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 8
DT = 5.0
T, E, K, C, L = 128, 2, 4, 16, 64
AXES = [("rod", "rate"), ("valve", "rate"), ("flow", "rate"), (None, "value")]
GAMMA, LAM, EPS = 0.99, 0.95, 1e-8
BATCH = 65536
REPS = 4      # epochs in one timed window
PEAK_BYTES_PER_S = 8.0e12


def columns():
    from nuclear_sim_amd.env import INFO_COLUMNS
    return ([("obs", i) for i in range(8)] + [("info", name) for name in INFO_COLUMNS[:4]] +
            ["reward", ("pump.oil_level", 0), ("pump.oil_level", 1), "prim.fuel_temperature"])[:C]


def row_bytes():
    """bytes one transition takes through a minibatch: every gathered row once in and once out, and its index"""
    return 2 * 4 * (K * C + len(AXES) + E + 1 + 1) + 4


def by_hand_epochs(torch, r, adv, ret, n, epochs, keep=False):
    """epochs the way a user does them today, mean and std once as the device forms its moments once; `keep`: the normalised advantages
    of the whole rollout instead of the last minibatch, for the comparison of bits"""
    mean, std = adv.mean(), adv.std()
    last = None
    for _ in range(epochs):
        last = by_hand_epoch(torch, r, adv, ret, n, mean, std)
    if keep:
        return (adv - mean) / (std + EPS), torch.stack([mean.double(), std.double()])
    return last


def by_hand_epoch(torch, r, adv, ret, n, mean, std):
    N = T * n
    perm = torch.randperm(N, device=adv.device)
    obs, act, extra = r["obs"].view(N, K, C), r["act"].view(N, len(AXES)), r["extra"].view(N, E)
    a, q = adv.reshape(N), ret.reshape(N)
    last = None
    for first in range(0, N, BATCH):
        idx = perm[first:first + BATCH]
        last = (obs.index_select(0, idx), act.index_select(0, idx), extra.index_select(0, idx),
                (a.index_select(0, idx) - mean) / (std + EPS), q.index_select(0, idx))
    return last


def measure(n, rounds, only_off, calls):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, noise_generator="device", autoreset=True, max_episode_steps=L)
    env.set_features(columns(), stack=K, final=True)
    env.set_controls(AXES)
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    env.controls_input().copy_(((torch.rand((n, len(AXES)), generator=g) * 2.0 - 1.0) * 0.02).to(torch.float32))
    x = env.controls_input()
    extras = (torch.rand((n, E), generator=g) - 0.5).to(device=dev, dtype=torch.float32)
    env.features()
    env.set_rollout(T, extras=E)
    env.rollout_extras_input().copy_(extras)

    def timed(work):      # one window: us
        return time_steps(stream, work, 1)

    def horizon(steps=T):
        for _ in range(steps):
            x.neg_()      # the policy's new output
            env.step()
    # off: blocks of one horizon with the rollout recording, nothing of the feature called
    off = []
    for k in range(1 + rounds):
        env.rollout_begin()
        horizon(W)
        env.rollout_begin()
        us = timed(horizon) / T
        if k:
            off.append(us)
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": T, "rounds": rounds,
           "features": [K, C], "axes": len(AXES), "extras": E, "max_episode_steps": L, "setups": {"off": stats(off)}}
    if not only_off:
        r = env.rollout()      # (the last block left a full horizon)
        assert r["t"] == T
        R = env.rollout_spec()["final_rows"]
        last = (torch.rand(n, generator=g) - 0.5).to(device=dev, dtype=torch.float32)
        final = (torch.rand(n * R, generator=g) - 0.5).to(device=dev, dtype=torch.float32)
        adv, ret = env.rollout_advantages(GAMMA, LAM, values=("extra", 0), last_value=last, final_values=final)
        N, plants = T * n, BATCH // T
        made = {}

        def device_epoch(unit, batch):
            def work():
                made[unit] = sum(1 for _ in env.rollout_minibatches(batch, epochs=REPS, seed=1, first_epoch=REPS * len(epochs[unit]), eps=EPS,
                                                                    unit=unit)) // REPS
            return work

        def hand():
            by_hand_epochs(torch, r, adv, ret, n, REPS)
        setups = {"device": device_epoch("transition", BATCH), "plant": device_epoch("plant", plants),
                  "by_hand_a": hand, "by_hand_b": hand}
        epochs = {"transition": [], "plant": []}
        names = list(setups)
        for s in names:      # warm-up: every shape the timed window uses
            timed(setups[s])
        times = {s: [] for s in names}
        for k in range(rounds):
            for s in names[k % len(names):] + names[:k % len(names)]:
                times[s].append(timed(setups[s]) / REPS)
                if s in ("device", "plant"):
                    epochs["transition" if s == "device" else s].append(k)
        moments_us = [timed(lambda: env.rollout_moments()) for _ in range(W // 2 + calls)][W // 2:]
        minibatches = {"device": made["transition"], "plant": made["plant"], "by_hand_a": -(-N // BATCH), "by_hand_b": -(-N // BATCH)}
        ep = {s: stats(v) for s, v in times.items()}
        for s in names:
            ep[s]["minibatches"] = minibatches[s]
            ep[s]["per_minibatch_us"] = ep[s]["median_us"] / minibatches[s]
        for s in ("device", "plant"):
            ep[s]["bytes_per_minibatch"] = row_bytes() * BATCH
            ep[s]["achieved_bytes_per_s"] = ep[s]["bytes_per_minibatch"] / (ep[s]["per_minibatch_us"] * 1e-6)
            ep[s]["share_of_8_TB_per_s"] = ep[s]["achieved_bytes_per_s"] / PEAK_BYTES_PER_S
        hand = min(ep["by_hand_a"]["median_us"], ep["by_hand_b"]["median_us"])
        spread = abs(ep["by_hand_a"]["median_us"] - ep["by_hand_b"]["median_us"])
        # the bits: torch's normalised advantages against the device's, through one minibatch that holds every transition
        normal, torch_moments = by_hand_epochs(torch, r, adv, ret, n, 1, keep=True)
        m = env.rollout_moments()
        whole = next(iter(env.rollout_minibatches(N, seed=1, eps=EPS)))
        diff = (whole["adv"].double() - normal.reshape(N).index_select(0, whole["index"].long()).double()).abs().max()
        tiled = bool(torch.equal(torch.sort(whole["index"]).values, torch.arange(N, dtype=torch.int32, device=dev)))
        out["epoch"] = {"transitions": N, "batch_size": BATCH, "plants_per_plant_minibatch": plants, "setups": ep,
                        "by_hand_us": hand, "by_hand_spread_us": spread, "by_hand_minus_device_us": hand - ep["device"]["median_us"],
                        "by_hand_minus_plant_us": hand - ep["plant"]["median_us"],
                        "device_epoch_is_below_by_hand": bool(hand - ep["device"]["median_us"] > spread),
                        "plant_epoch_is_below_by_hand": bool(hand - ep["plant"]["median_us"] > spread),
                        "largest_difference_of_the_normalised_advantages": float(diff.item()),
                        "moments_device": [float(v) for v in m.cpu()], "mean_std_torch": [float(v) for v in torch_moments.cpu()],
                        "the_epoch_tiles_the_transitions_exactly_once": tiled}
        out["moments"] = dict(stats(moments_us), rows=T, cols=n, launches=4)
    env.set_rollout(None)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="timed calls of rollout_moments")
    add_parent_arguments(ap, "minibatch_overhead.json")
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
    out = {"what": "over a recorded rollout of config 4 (device noise, autoreset, features of 16 columns x 4 frames float32, controls of 4 axes, "
                   "E = 2, T = 128): one epoch of shuffled minibatches of 65 536 transitions through rollout_minibatches, by transition and by "
                   "plant, against randperm + five index_selects + mean / std by hand in torch; rollout_moments alone; and the step with the "
                   "feature unused",
           "sizes": sizes, "head": head(ROOT)}
    write_line(out, a.out)


if __name__ == "__main__":
    main()
