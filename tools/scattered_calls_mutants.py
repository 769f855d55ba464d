#!/usr/bin/env python3
"""Which tests see a wrong operator-maintenance handler?  A hand-picked list of single-token mutants of the device code behind
npb_perform_maintenance / npb_perform_component_maintenance (npd_component_maintenance.h, the operator part of npb_kernels.hip, the
handlers of npd_maintenance.h), each a changed VALUE or COMPARISON -- none changes an address, a loop bound, a launch shape or a store --
built into its own libnpb.so as tools/mutate_device.py builds its mutants (only npb_kernels.hip's fp64 object is recompiled, so the
fp32-storage tests run the unmutated kernels) and run against

    old:  tests/test_component_maintenance_gpu.py tests/test_operator_maintenance_gpu.py      (the suite before the scattered calls)
    new:  tests/test_scattered_calls_gpu.py

    python3 tools/scattered_calls_mutants.py build [--jobs 8]     here (hipcc cross-compiles): tools/device_mutants/libnpb_sc<k>.so
    python3 tools/scattered_calls_mutants.py run [--jobs 6]       on the GPU box: verdicts into profiles/scattered_calls_mutants.json (--out)
"""
import argparse
import concurrent.futures as cf
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mutate_device import link_objects   # noqa: E402
CSRC = os.path.join(ROOT, "nuclear_sim_amd", "csrc")
BUILD = os.path.join(ROOT, "nuclear_sim_amd", "build")
OUT = os.path.join(ROOT, "tools", "device_mutants")
HIPFLAGS = "-O3 --offload-arch=gfx950 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -freciprocal-math -fapprox-func -fvisibility=hidden -w".split()
OLD = ["tests/test_component_maintenance_gpu.py", "tests/test_operator_maintenance_gpu.py"]
NEW = ["tests/test_scattered_calls_gpu.py"]
C, K, M = "npd_component_maintenance.h", "npb_kernels.hip", "npd_maintenance.h"

# (file, the text as it is -- it must occur exactly once --, the mutant's text, what it is)
MUTANTS = [
    (C, "g->tsp_copper[level] *= (1.0 - effectiveness * 0.8);", "g->tsp_copper[level] *= (1.0 - effectiveness * 0.9);", "TSP cleaning: copper factor 0.8 -> 0.9"),
    (C, "&& *cleaned < 2)", "&& *cleaned <= 2)", "load balancing: the first two above 5 % -> the first three"),
    (C, "g->tsp_ht_degradation > 0.05", "g->tsp_ht_degradation >= 0.05", "load balancing: above 5 % -> at or above"),
    (C, "if (g->steam_quality < 0.99)", "if (g->steam_quality <= 0.99)", "system steam quality: below 0.99 -> at or below"),
    (C, "double quality_improvement = 0.999 - current_quality;", "double quality_improvement = 0.9995 - current_quality;", "moisture separator: aims at 0.999 -> 0.9995"),
    (C, "scale_removal = 0.4; corrosion_removal = 0.9; }", "scale_removal = 0.4; corrosion_removal = 0.8; }", "condenser cleaning, hydroblast: corrosion removal 0.9 -> 0.8"),
    (C, "cd->corrosion_product_thickness *= 0.7;", "cd->corrosion_product_thickness *= 0.8;", "water treatment: corrosion products 0.7 -> 0.8"),
    (C, "g->scale_thickness = npd_pymax(0.0, g->scale_thickness);", "g->scale_thickness = (g->scale_thickness);", "scale cleaning: npd_pymax(0.0, x) -> x"),
    (C, "cd->ej_nozzle_erosion[e] = npd_pymin(1.0, cd->ej_nozzle_erosion[e] + 0.1);", "cd->ej_nozzle_erosion[e] = npd_pymin(1.0, cd->ej_nozzle_erosion[e] + 0.2);",
     "ejector mechanical cleaning: erosion + 0.1 -> + 0.2"),
    (C, "cd->ej_diffuser_fouling[e] = npd_pymin(1.0, cd->ej_diffuser_fouling[e] + 0.4);", "cd->ej_diffuser_fouling[e] = (cd->ej_diffuser_fouling[e] + 0.4);",
     "ejector chemical cleaning: the diffuser's cap at 1.0 dropped"),
    (C, "return option == NPB_CLEANING_DEFAULT ? NPB_CLEANING_CHEMICAL : option;", "return option <= NPB_CLEANING_DEFAULT ? NPB_CLEANING_CHEMICAL : option;",
     "cleaning type: a negative option taken for the default"),
    (K, "if (unit == e) npd_ejector_maintenance(&cd, e, action, option);", "if (unit != e) npd_ejector_maintenance(&cd, e, action, option);", "the other ejector is serviced"),
    (K, "if (kind == NPB_COMPONENT_SGSYS || kind == NPB_COMPONENT_COND) unit = 0;", "if (kind == NPB_COMPONENT_SGSYS || kind == NPB_COMPONENT_COND) unit = unit;",
     "system and condenser actions no longer ignore the unit"),
    (K, "double target_level = 95.0;", "double target_level = 90.0;", "oil top-off: default target 95.0 -> 90.0"),
    (K, "bearing > NPB_BEARING_THRUST)) ok = false;", "bearing >= NPB_BEARING_THRUST)) ok = false;", "bearing replacement: the thrust bearing refused"),
    (M, "p->oil_level = npd_pymin(100.0, target_level);", "p->oil_level = (target_level);", "oil top-off: the cap at 100 % dropped"),
    (M, "if (p->wear_motor_bearings > 3.0) { p->wear_motor_bearings *= 0.95;", "if (p->wear_motor_bearings > 3.0) { p->wear_motor_bearings *= 0.9;",
     "motor inspection: 0.95 -> 0.9"),
    (M, "double contamination_reduction = npd_pymin(old_contamination * 0.7, 50.0);", "double contamination_reduction = npd_pymin(old_contamination * 0.6, 50.0);",
     "system cleaning: contamination 0.7 -> 0.6"),
]


def build_one(k):
    name, was, now, what = MUTANTS[k]
    work = tempfile.mkdtemp(prefix="npd_scmut_")
    try:
        os.makedirs(os.path.join(work, "nuclear_sim_amd"))
        shutil.copytree(CSRC, os.path.join(work, "nuclear_sim_amd", "csrc"))       # the headers include ../../include/ by relative path
        os.symlink(os.path.join(ROOT, "include"), os.path.join(work, "include"))
        path = os.path.join(work, "nuclear_sim_amd", "csrc", name)
        text = open(path).read()
        rec = {"k": k, "file": name, "line": text[:text.find(was)].count("\n") + 1, "was": was, "now": now, "what": what}
        if text.count(was) != 1:
            rec["build"] = "the text occurs %d times" % text.count(was)
            return rec
        open(path, "w").write(text.replace(was, now))
        obj = os.path.join(work, "k64.o")
        cc = subprocess.run(["/opt/rocm/bin/hipcc"] + HIPFLAGS + ["-c", "-o", obj, os.path.join(work, "nuclear_sim_amd", "csrc", "npb_kernels.hip")],
                            capture_output=True, text=True)
        if cc.returncode != 0:
            rec["build"] = "stillborn"
            return rec
        so = os.path.join(OUT, "libnpb_sc%d.so" % k)
        ld = subprocess.run(["/opt/rocm/bin/hipcc"] + HIPFLAGS + ["-shared", "-pthread", "-o", so, obj] + link_objects(), capture_output=True, text=True)
        rec["build"] = "ok" if ld.returncode == 0 else "link failed"
        return rec
    finally:
        shutil.rmtree(work, ignore_errors=True)


def cmd_build(args):
    for f in link_objects():
        if not os.path.exists(f):
            sys.exit("build the product library first (make -C nuclear_sim_amd/csrc): %s is missing" % f)
    os.makedirs(OUT, exist_ok=True)
    out = []
    with cf.ProcessPoolExecutor(args.jobs) as pool:
        for rec in pool.map(build_one, range(len(MUTANTS))):
            out.append(rec)
            print("%2d %-30s %4d build %-10s %s" % (rec["k"], rec["file"], rec["line"], rec["build"], rec["what"]), flush=True)
    json.dump(out, open(os.path.join(OUT, "scattered_calls_index.json"), "w"), indent=1)


def cmd_run(args):
    index = json.load(open(os.path.join(OUT, "scattered_calls_index.json")))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    stop = threading.Event()        # a run that ends in anything but pytest's "passed" / "tests failed" ends the whole measurement

    def one(job):
        rec, which, files = job
        if stop.is_set():
            return rec, which, "not run", ""
        env = dict(os.environ, NPB_LIB=os.path.join(OUT, "libnpb_sc%d.so" % rec["k"]), PYTHONDONTWRITEBYTECODE="1")
        try:
            t = subprocess.run([sys.executable, "-m", "pytest"] + files + ["-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                               capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            stop.set()
            return rec, which, "timeout", ""
        if t.returncode not in (0, 1):
            stop.set()
            return rec, which, "exit status %d" % t.returncode, t.stdout[-300:]
        m = re.search(r"FAILED (\S+)", t.stdout)
        return rec, which, "survived" if t.returncode == 0 else "killed", (m.group(1) if m else "")
    jobs = [(rec, which, files) for rec in index if rec["build"] == "ok" for which, files in (("new", NEW), ("old", OLD))]
    with cf.ThreadPoolExecutor(args.jobs) as pool:
        for rec, which, verdict, by in pool.map(one, jobs):
            rec[which] = verdict
            if by:
                rec[which + "_by"] = by
            print("%2d %-30s %-4s %-9s %s" % (rec["k"], rec["file"], which, verdict, by), flush=True)
            json.dump({"old_files": OLD, "new_files": NEW, "mutants": index}, open(args.out, "w"), indent=1)
    done = [r for r in index if "new" in r and "old" in r]
    print("%d mutants: the new file kills %d, the old files %d; alive in the old files: %s" % (
        len(done), sum(r["new"] == "killed" for r in done), sum(r["old"] == "killed" for r in done), [r["k"] for r in done if r["old"] == "survived"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["build", "run"])
    ap.add_argument("--jobs", type=int, default=6)
    ap.add_argument("--timeout", type=int, default=420, help="run: seconds per pytest run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scattered_calls_mutants.json"), help="run: where the table goes")
    a = ap.parse_args()
    (cmd_build if a.cmd == "build" else cmd_run)(a)
