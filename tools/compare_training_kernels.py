"""The policy's and the training path's kernels of this tree against another checkout's: resource tables side by side, and which are the same text.

    python tools/compare_training_kernels.py OTHER_TREE [--keep DIR]

Compiles npb_policy.hip, npb_policy_core.hip, npb_ppo.hip and npb_ppo_seq.hip of both trees for the device only, each with its tree's own
NOISEFLAGS (csrc/Makefile: the line those units are built with) plus -S -Rpass-analysis=kernel-resource-usage, and prints one row per kernel:
VGPRs, AGPRs, scratch, VGPR spills, scalars spilled into VGPR lanes, occupancy and LDS of the other tree and of this one, and whether the
assembly text is the same (compare_step_kernels.functions does the normalising).  Exit status 1 where a kernel of this tree has scratch, a
VGPR spill, another occupancy or LDS size than the other tree's, or more VGPRs (npb_ppo_seq_kernel, which sits at the limit: more than 256);
or where a kernel of npb_policy.hip or npb_ppo.hip differs in text.  Needs hipcc, no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile

from compare_step_kernels import ROOT, functions, resources

UNITS = ("npb_policy.hip", "npb_policy_core.hip", "npb_ppo.hip", "npb_ppo_seq.hip")
SAME_TEXT = ("npb_policy.hip", "npb_ppo.hip")
FIGURES = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch"), ("VGPRs Spill", "vspill"), ("SGPRs Spill", "sspill"),
           ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "LDS"))


def noiseflags(tree):
    text = open(os.path.join(tree, "nuclear_sim_amd", "csrc", "Makefile")).read().replace("\\\n", " ")
    arch = re.search(r"^ARCH \?= *(\S+)", text, flags=re.M).group(1)
    return re.search(r"^NOISEFLAGS \?= *(.*)$", text, flags=re.M).group(1).replace("$(ARCH)", arch).split()


def start(tree, out):
    jobs = []
    for unit in UNITS:
        stem = os.path.join(out, unit[:-len(".hip")])
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + noiseflags(tree) + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                                                     "-o", stem + ".s", unit]
        with open(stem + ".remarks", "w") as f:
            jobs.append((subprocess.Popen(cmd, cwd=os.path.join(tree, "nuclear_sim_amd", "csrc"), stderr=f), unit, stem))
    return jobs


def table(jobs):
    out = {}
    for p, unit, stem in jobs:
        if p.wait() != 0:
            raise SystemExit("compiling %s failed: see %s.remarks" % (unit, stem))
        text, res = functions(stem + ".s"), resources(stem + ".remarks")
        for name, rows in res.items():
            figures = {}
            for row in rows:
                key, _, value = row.rpartition(": ")
                figures[key] = int(value) if value.isdigit() else value
            out[name] = (unit, figures, text.get(name))
    return out


def main(argv):
    other = argv[0]
    keep = argv[argv.index("--keep") + 1] if "--keep" in argv else tempfile.mkdtemp(prefix="npb_train_cmp_")
    started = {}
    for tag, tree in (("other", other), ("this", ROOT)):
        os.makedirs(os.path.join(keep, tag), exist_ok=True)
        started[tag] = start(tree, os.path.join(keep, tag))
    a, b = table(started["other"]), table(started["this"])
    bad = []
    print("every figure: other tree / this tree")
    print("%-9s %-9s %-7s %-7s %-9s %-5s %-17s %-9s %s" % tuple([short for _, short in FIGURES] + ["text", "kernel"]))
    for name in sorted(set(a) | set(b), key=lambda k: ((a.get(k) or b.get(k))[0], k)):
        if name not in a or name not in b:
            print("%s: only in %s" % (name, "the other tree" if name in a else "this tree"))
            bad.append(name)
            continue
        (unit, fa, ta), (_, fb, tb) = a[name], b[name]
        same = ta == tb
        print("%-9s %-9s %-7s %-7s %-9s %-5s %-17s %-9s %s (%s)" % tuple(["%s/%s" % (fa.get(key), fb.get(key)) for key, _ in FIGURES] +
                                                                          ["same" if same else "differs", name, unit]))
        most = 256 if "npb_ppo_seq_kernel" in name else fa.get("VGPRs")      # (the sequence kernel sits at the register limit in both builds)
        if fb.get("ScratchSize [bytes/lane]") or fb.get("VGPRs Spill") or fb.get("VGPRs") > most or (unit in SAME_TEXT and not same) or \
                any(fa.get(key) != fb.get(key) for key in ("Occupancy [waves/SIMD]", "LDS Size [bytes/block]")):
            bad.append(name)
    print("outside the rule:", bad if bad else "none")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
