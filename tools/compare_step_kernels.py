"""Are the step kernels of this tree, instruction for instruction, those of another checkout?

    python tools/compare_step_kernels.py OTHER_TREE [--keep DIR]

Compiles nuclear_sim_amd/csrc/npb_kernels.hip of both trees for the device only (each tree's own HIPFLAGS, read from its
csrc/Makefile, -S, both storage builds) with -Rpass-analysis=kernel-resource-usage, and compares every function whose name contains "npb_step" or "npd_maint_rule_for_wave" -- the
step kernels bench.py times and the rule they call -- by its assembly text (comments and debug directives dropped; local labels
.LBB<f>_<n> / .Ltmp<n> stripped of the function's ordinal in the file, which moves when a kernel is added elsewhere) and by its
resource table (registers, spills, scratch, occupancy, LDS).  Lists the other functions that changed or are new.  Exit status 1 if a
step kernel differs.  Needs hipcc, no GPU.
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


def compile_tree(tree, out, storage):
    src = os.path.join(tree, "nuclear_sim_amd", "csrc")
    asm, rem = os.path.join(out, storage + ".s"), os.path.join(out, storage + ".remarks")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + makefile_flags(tree) + (["-DNPB_BUILD_F32"] if storage == "f32" else []) + ["-o", asm, "npb_kernels.hip"]
    with open(rem, "w") as f:
        return subprocess.Popen(cmd, cwd=src, stderr=f), asm, rem


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
            jobs[(tag, st)] = compile_tree(tree, d, st)
    for (tag, st), (p, _a, _r) in jobs.items():
        if p.wait() != 0:
            raise SystemExit("compiling the %s tree (%s) failed: see %s" % (tag, st, jobs[(tag, st)][2]))
    bad = 0
    for st in ("f64", "f32"):
        a, b = functions(jobs[("other", st)][1]), functions(jobs[("this", st)][1])
        ra, rb = resources(jobs[("other", st)][2]), resources(jobs[("this", st)][2])
        step = sorted(k for k in a if "npb_step" in k or "npd_maint_rule_for_wave" in k)
        differ = [k for k in step if k not in b or a[k] != b[k] or ra.get(k) != rb.get(k)]
        bad += len(differ)
        print("%s storage: %d step kernels and rule instantiations, %d instructions and directives: %s" % (
            st, len(step), sum(len(a[k].splitlines()) for k in step), "identical, resource tables too" if not differ else "DIFFERENT: %s" % differ))
        print("  other functions changed:", sorted(k for k in a if k not in step and (k not in b or a[k] != b[k] or ra.get(k) != rb.get(k))))
        print("  new functions:", sorted(k for k in b if k not in a))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
