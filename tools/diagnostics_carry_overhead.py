"""What carrying the diagnostics rows through the restores costs: the episode and restore kernels take one more side pointer
(npd_restore_side_t.dg), NULL unless npb_carry_diagnostics is on.

    python tools/diagnostics_carry_overhead.py --parent OTHER_TREE [--rounds 5] [--blocks 4] [--block 200]

Feature off (no diagnostics), this tree against OTHER_TREE -- a built checkout of the parent commit -- on the same box in one session:
worker processes alternate between the two trees, `--rounds` of each, and each worker times `--blocks` blocks of `--block` event-timed
steps of tools/autoreset_overhead.py's three cases on ONE handle at 65 536 plants, after 200 warm-up launches of each:
  on_idle   autoreset on, nobody resets
  on_1pct   autoreset on, max_episode_steps = 100 with staggered counters: ~1 % of the plants reset per step
  on_all    autoreset on, max_episode_steps = 1: every plant resets on every step
(a worker is a process of its own because two builds of libnpb.so do not share one; where a handle's arena lands moves its step time,
npb_api.hip probe_placement, which is why each tree gets several handles and they alternate).  The gate: this tree's median per case
lies within the parent's own interquartile range of the session.  Then the carrying cost, reported and not gated: the same cases on
this tree with diagnostics=True (the diagnostics build of the step kernel, meant for logging), against diagnostics on without
autoreset.  One JSON line, written to --out.
"""
import argparse
import json
import os
import sys

from overhead_harness import fresh_process, head, stats, time_steps, write_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX = 100
CASES = ("on_idle", "on_1pct", "on_all")


def worker(a):
    sys.path.insert(0, os.path.abspath(a.worker))
    import torch
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = a.n
    env = BatchedPlantEnv(n, autoreset=True, **({"diagnostics": True} if a.diagnostics else {}))
    L, h, dev = env.L, env._h, env.device
    lane = torch.arange(n, device=dev)
    stream = torch.cuda.current_stream(dev)

    def prepare(name):
        if name == "off":
            _lib.check(L.npb_set_autoreset(h, 0, 0), h)
        elif name == "on_idle":
            _lib.check(L.npb_set_autoreset(h, 1, 0), h)
        elif name == "on_1pct":      # plant p's counter at (k - p) mod MAX
            _lib.check(L.npb_set_autoreset(h, 1, MAX), h)
            for k in range(MAX):
                env.step()
                env.restore(lane % MAX == k)
        elif name == "on_all":
            _lib.check(L.npb_set_autoreset(h, 1, 1), h)

    def run_block(steps):
        return time_steps(stream, env.step, steps)

    cases = (("off",) if a.diagnostics else ()) + CASES
    for name in cases:
        prepare(name)
        run_block(200)
    times = {c: [] for c in cases}
    for _ in range(a.blocks):
        for name in cases:
            prepare(name)
            times[name].append(run_block(a.block))
    info = {"times_us": times, "step_kernel": env.last_step_kernel(), "device": torch.cuda.get_device_name(dev)}
    env.close()
    print(json.dumps(info))      # the worker's last line: what fresh_process reads


def run_worker(a, tree, diagnostics):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", tree, "--n", str(a.n), "--blocks", str(a.blocks), "--block", str(a.block)]
    if diagnostics:
        cmd.append("--diagnostics")
    return fresh_process(cmd, a.worker_timeout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--block", type=int, default=200)
    ap.add_argument("--carry-rounds", type=int, default=2)
    ap.add_argument("--worker-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diagnostics_carry_overhead.json"))
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    ap.add_argument("--diagnostics", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent:
        ap.error("--parent OTHER_TREE is needed: the feature-off cost is measured against the parent commit in the same session")
    times = {"parent": {c: [] for c in CASES}, "this": {c: [] for c in CASES}}
    meta = {}
    for r in range(a.rounds):
        for who, tree in (("parent", a.parent), ("this", ROOT)) if r % 2 == 0 else (("this", ROOT), ("parent", a.parent)):
            w = run_worker(a, tree, False)
            meta = {"step_kernel": w["step_kernel"], "device": w["device"]}
            for c in CASES:
                times[who][c] += w["times_us"][c]
    carry = {c: [] for c in ("off",) + CASES}
    carry_kernel = None
    for r in range(a.carry_rounds):
        w = run_worker(a, ROOT, True)
        carry_kernel = w["step_kernel"]
        for c in carry:
            carry[c] += w["times_us"][c]
    off = {who: {c: stats(v) for c, v in t.items()} for who, t in times.items()}
    gate = {c: bool(off["parent"][c]["p25_us"] <= off["this"][c]["median_us"] <= off["parent"][c]["p75_us"]) for c in CASES}
    below = {c: bool(off["this"][c]["median_us"] < off["parent"][c]["p25_us"]) for c in CASES}
    res = {"what": "per-step time of npb_step with autoreset: diagnostics off, this tree against the parent commit in alternating worker "
                   "processes of one session; and with the diagnostics rows carried (diagnostics=True), this tree",
           "n_plants": a.n, "block_steps": a.block, "blocks_per_worker": a.blocks, "rounds": a.rounds, "max_episode_steps_1pct": MAX,
           "diagnostics_off": dict(off, **meta),
           "this_median_within_parent_iqr": gate, "this_median_below_parent_p25": below,
           "diagnostics_carried": {"step_kernel": carry_kernel, "setups": {c: stats(v) for c, v in carry.items()} if a.carry_rounds else {}},
           "head": head(ROOT)}
    if a.carry_rounds:
        o = res["diagnostics_carried"]["setups"]["off"]["median_us"]
        res["diagnostics_carried"]["overhead_vs_no_autoreset_pct"] = {c: 100.0 * (res["diagnostics_carried"]["setups"][c]["median_us"] / o - 1.0) for c in CASES}
    write_line(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
