"""Are the step kernels of this tree, instruction for instruction, those of another checkout?  And every other kernel built with their flags?

    python tools/compare_step_kernels.py OTHER_TREE [--keep DIR]

Compiles, of both trees, every unit that the tree's csrc/Makefile builds with HIPFLAGS through its two pattern rules (the <unit>_f64.o and
<unit>_f32.o of `make print-objects`; a tree without that target builds npb_kernels.hip alone that way) for the device only (each tree's own
HIPFLAGS, read from its csrc/Makefile, -S) with -Rpass-analysis=kernel-resource-usage, and pools the functions per storage build: which
unit a function lives in is not compared.  Every function whose name contains "npb_step" or "npd_maint_rule_for_wave" -- the
step kernels bench.py times and the rule they call -- is compared by its assembly text (comments and debug directives dropped; local labels
.LBB<f>_<n> / .Ltmp<n> stripped of the function's ordinal in the file, which moves when a kernel is added elsewhere) and by its
resource table (registers, spills, scratch, occupancy, LDS).  So is every other pooled function: the changed, the new and the lost ones are
listed.  Exit status 1 if a step kernel differs.  Needs hipcc and make, no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def makefile_flags(tree):
    """HIPFLAGS of the tree's own csrc/Makefile (its one definition; $(ARCH) expanded), plus what this comparison needs"""
    text = open(os.path.join(tree, "nuclear_sim_amd", "csrc", "Makefile")).read().replace("\\\n", " ")
    arch = re.search(r"^ARCH \?= *(\S+)", text, flags=re.M).group(1)
    flags = re.search(r"^HIPFLAGS \?= *(.*)$", text, flags=re.M).group(1).replace("$(ARCH)", arch).split()
    return flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]


def makefile_objects(tree):
    """the tree's object list as its csrc/Makefile prints it (`make print-objects`), or None for a tree whose Makefile has no such target"""
    make = subprocess.run(["make", "-s", "-C", os.path.join(tree, "nuclear_sim_amd", "csrc"), "print-objects"], capture_output=True, text=True)
    return make.stdout.split() if make.returncode == 0 else None


def units(tree, storage):
    """the sources the tree's Makefile compiles with HIPFLAGS for this storage build"""
    objects = makefile_objects(tree)
    if objects is None:
        return ["npb_kernels.hip"]
    return [o[:-len("_%s.o" % storage)] + ".hip" for o in objects if o.endswith("_%s.o" % storage)]


def compile_unit(tree, out, storage, unit):
    src = os.path.join(tree, "nuclear_sim_amd", "csrc")
    stem = os.path.join(out, "%s_%s" % (unit[:-len(".hip")], storage))
    asm, rem = stem + ".s", stem + ".remarks"
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + makefile_flags(tree) + (["-DNPB_BUILD_F32"] if storage == "f32" else []) + ["-o", asm, unit]
    with open(rem, "w") as f:
        return subprocess.Popen(cmd, cwd=src, stderr=f), asm, rem


def pooled(jobs):
    """the functions and resource tables of one tree's units of one storage build, as one pool each"""
    fn, res = {}, {}
    for _p, asm, rem in jobs:
        for k, v in functions(asm).items():
            if k in fn:
                raise SystemExit("%s is defined by two units of one build: %s" % (k, asm))
            fn[k] = v
        res.update(resources(rem))
    return fn, res


def functions(path):
    out = {}
    for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n(.*?)^\s*\.size\s+\1,", open(path).read(), flags=re.S | re.M):
        lines = [ln.split(";")[0].rstrip() for ln in m.group(2).splitlines()]
        body = "\n".join(ln for ln in lines if ln.strip() and not ln.strip().startswith((".loc", ".file", ".cfi", "//")))
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        out[m.group(1)] = re.sub(r"\.L(tmp|func_begin|func_end|JTI|post_getpc|pcsections)\d+(_\d+)?", r".L\1", body)
    return out


def resources(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.search(r"remark: .*Function Name: (\S+)", ln)
        if m:
            cur = m.group(1); out[cur] = []
            continue
        m = re.search(r"remark: (?:[^:\s]*:\d+:\d+: )?\s*(.*?)\s*\[-Rpass-analysis", ln)      # (the location leads the line, or follows "remark:")
        if m and cur:
            out[cur].append(m.group(1).strip())
    return out


def main(argv):
    other = argv[0]
    keep = argv[argv.index("--keep") + 1] if "--keep" in argv else tempfile.mkdtemp(prefix="npb_cmp_")
    jobs = {}
    for tag, tree in (("other", other), ("this", ROOT)):
        for st in ("f64", "f32"):
            d = os.path.join(keep, tag); os.makedirs(d, exist_ok=True)
            jobs[(tag, st)] = [compile_unit(tree, d, st, unit) for unit in units(tree, st)]
    for (tag, st), started in jobs.items():
        for p, _a, rem in started:
            if p.wait() != 0:
                raise SystemExit("compiling the %s tree (%s) failed: see %s" % (tag, st, rem))
    bad = 0
    for st in ("f64", "f32"):
        (a, ra), (b, rb) = pooled(jobs[("other", st)]), pooled(jobs[("this", st)])
        step = sorted(k for k in a if "npb_step" in k or "npd_maint_rule_for_wave" in k)
        differ = [k for k in step if k not in b or a[k] != b[k] or ra.get(k) != rb.get(k)]
        bad += len(differ)
        print("%s storage: %d step kernels and rule instantiations, %d instructions and directives: %s" % (
            st, len(step), sum(len(a[k].splitlines()) for k in step), "identical, resource tables too" if not differ else "DIFFERENT: %s" % differ))
        same = [k for k in a if k in b and a[k] == b[k] and ra.get(k) == rb.get(k)]
        print("  all functions of %s: %d in the other tree, %d in this one, %d identical in text and resource table" % (
            ", ".join(units(ROOT, st)), len(a), len(b), len(same)))
        print("  other functions changed:", sorted(k for k in a if k not in step and k in b and (a[k] != b[k] or ra.get(k) != rb.get(k))))
        print("  new functions:", sorted(k for k in b if k not in a))
        print("  lost functions:", sorted(k for k in a if k not in b))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
