"""The measuring parts that the tools/*_overhead.py scripts share: plain functions, called by scripts that stay scripts.

Why a measurement here is made the way it is:
  one handle per size   where an arena lands in physical memory moves the step time from one handle to the next (npb_api.hip,
                        probe_placement), so two handles compared would measure placement.  A script builds one env per size and
                        switches its feature on and off on that env between blocks.
  event-timed blocks    a block is N steps between two device events and ends in a synchronise on the closing event (time_steps):
                        without it the elapsed time is read before the work is done.
  the rotation          order effects exist -- what ran before a block moves its time -- so after one warm-up block of every setup the
                        order of the setups rotates from round to round (rotated_blocks), and a feature's cost is the difference of the
                        two blocks of the SAME round (paired).
  fresh processes       two builds of libnpb.so do not share a process, so the parent commit's build is measured by running the same
                        script in processes of their own, alternately on this build and on the parent's (off_across_builds), and
                        bench.py from the two trees in turn (bench_alternated).
  a child that failed   nothing is started after it: fresh_process raises SystemExit on a non-zero exit status and on a time limit, and
                        every child of every script goes through it.
  the agreement rule    whether `off` agrees with the parent's is stated once, in compare_off, and nowhere else.

Nothing of nuclear_sim_amd is imported here: --package-root decides where the package comes from.  torch is imported only in time_steps.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def time_steps(stream, step, steps):
    """`steps` calls of step() between two events on `stream`: us per call, read after a synchronise on the closing event"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(steps):
        step()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def rotated_blocks(setups, rounds, run_block):
    """one warm-up block of every setup, then `rounds` rounds in an order that rotates with the round: {setup: [run_block(setup), ...]}"""
    setups = list(setups)
    for s in setups:      # warm-up
        run_block(s)
    blocks = {s: [] for s in setups}
    for r in range(rounds):
        k = r % len(setups)
        for s in setups[k:] + setups[:k]:
            blocks[s].append(run_block(s))
    return blocks


def stats(v):
    v = np.asarray(v)
    return {"median_us": float(np.median(v)), "p25_us": float(np.percentile(v, 25)), "p75_us": float(np.percentile(v, 75)),
            "min_us": float(v.min()), "max_us": float(v.max()), "blocks": int(v.size)}


def paired(blocks, a, b):
    d = np.asarray(blocks[a]) - np.asarray(blocks[b])      # the same round's blocks
    return {"median": float(np.median(d)), "min": float(d.min()), "max": float(d.max())}


def fresh_process(cmd, timeout, cwd=None):
    """run cmd in a process of its own and return the last line of its stdout, parsed as JSON.  A non-zero exit status or the time limit
    raises SystemExit after the tails of its output: the caller starts nothing further"""
    def text(s):
        return s.decode(errors="replace") if isinstance(s, bytes) else (s or "")
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=cwd)
    except subprocess.TimeoutExpired as e:
        sys.stderr.write(text(e.stdout)[-2000:] + text(e.stderr)[-4000:])
        raise SystemExit("%s ran past its limit of %s s" % (" ".join(cmd), timeout))
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("%s failed with status %d" % (" ".join(cmd), p.returncode))
    lines = p.stdout.strip().splitlines()
    if not lines:
        raise SystemExit("%s printed no result" % " ".join(cmd))
    return json.loads(lines[-1])


def off_across_builds(script, argv, parent, repeats, pick, timeout):
    """`script argv --package-root ROOT --only-off --out ""` in fresh processes: this build, the parent's, this build, the parent's ...,
    `repeats` times each.  Returns the two lists of pick(result), this build's first"""
    runs = {"this": [], "parent": []}
    for _ in range(repeats):
        for which, root in (("this", ROOT), ("parent", os.path.abspath(parent))):
            cmd = [sys.executable, os.path.abspath(script)] + [str(x) for x in argv] + ["--package-root", root, "--only-off", "--out", ""]
            runs[which].append(pick(fresh_process(cmd, timeout)))
            print("%s: off of the %s build in a fresh process" % (" ".join(str(x) for x in argv), which), file=sys.stderr, flush=True)
    return runs["this"], runs["parent"]


def compare_off(this_medians, parent_medians, handle_stats):
    """THE agreement rule.  Fresh processes only on both sides, like against like; off agrees with the parent's if the medians of the two
    differ by no more than the run-to-run spread: the largest of this build's processes', the parent's processes' and the blocks' of the
    handle that measured the feature (handle_stats: its stats() of the same setup).  The parent's own spread judges alone beside it"""
    this_spread = max(this_medians) - min(this_medians)
    parent_spread = max(parent_medians) - min(parent_medians)
    spread = max(this_spread, parent_spread, handle_stats["max_us"] - handle_stats["min_us"])
    diff = float(np.median(parent_medians) - np.median(this_medians))
    return {"this_medians_us": list(this_medians), "parent_medians_us": list(parent_medians), "parent_minus_this_us": diff,
            "this_spread_us": float(this_spread), "parent_spread_us": float(parent_spread), "spread_us": float(spread),
            "off_agrees": bool(abs(diff) <= spread), "off_within_the_parents_own_spread": bool(abs(diff) <= parent_spread)}


def bench_alternated(parent, repeats, steps, warmup, timeout=900):
    """bench.py from this tree and from the parent's, alternately: ms per step of each run"""
    runs = {"this": [], "parent": []}
    for _ in range(repeats):
        for which, root in (("this", ROOT), ("parent", os.path.abspath(parent))):
            cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
            runs[which].append(fresh_process(cmd, timeout, cwd=root)["ms_per_step"])
    return {"steps": steps, "warmup": warmup, "this_ms_per_step": runs["this"], "parent_ms_per_step": runs["parent"],
            "parent_minus_this_ms": float(np.median(runs["parent"]) - np.median(runs["this"]))}


def head(root):
    """the short commit id of the tree the script runs from, or None"""
    try:
        return subprocess.run(["git", "-C", root, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def write_line(out, path):
    """one JSON line to stdout and, unless path is empty, to path"""
    line = json.dumps(out)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


def add_parent_arguments(ap, out_name):
    """the flags of a script that compares `off` with the parent commit's build"""
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: `off` (and bench.py, where the script runs it) across the two builds")
    ap.add_argument("--process-repeats", type=int, default=2)
    ap.add_argument("--package-root", default=ROOT, help="where nuclear_sim_amd is imported from (used for the parent's build)")
    ap.add_argument("--only-off", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name))
