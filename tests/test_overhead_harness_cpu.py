"""tools/overhead_harness.py: the pure parts of the measuring harness, and the command lines of the 21 scripts written on it.  No GPU."""
import importlib.util
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
_spec = importlib.util.spec_from_file_location("overhead_harness", os.path.join(TOOLS, "overhead_harness.py"))      # (tools/ stays off sys.path)
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)


def test_stats():
    assert H.stats([1, 2, 3, 4, 10]) == {"median_us": 3.0, "p25_us": 2.0, "p75_us": 4.0, "min_us": 1.0, "max_us": 10.0, "blocks": 5}


def test_paired_takes_the_same_rounds_differences():
    blocks = {"on": [11.0, 14.0, 12.0, 20.0], "off": [10.0, 10.5, 11.5, 12.0]}      # differences 1, 3.5, 0.5, 8
    assert H.paired(blocks, "on", "off") == {"median": 2.25, "min": 0.5, "max": 8.0}
    assert H.paired(blocks, "off", "on") == {"median": -2.25, "min": -8.0, "max": -0.5}


def test_rotated_blocks_order():
    calls = []

    def run_block(s):
        calls.append(s)
        return float(len(calls))
    blocks = H.rotated_blocks(["a", "b", "c"], 4, run_block)
    assert "".join(calls) == "abc" + "abc" + "bca" + "cab" + "abc"
    assert set(blocks) == {"a", "b", "c"} and all(len(v) == 4 for v in blocks.values())
    # the warm-up blocks (calls 1..3) are not among the values; each value is its own call's
    assert blocks == {"a": [4.0, 9.0, 11.0, 13.0], "b": [5.0, 7.0, 12.0, 14.0], "c": [6.0, 8.0, 10.0, 15.0]}


HANDLE = {"median_us": 100.4, "p25_us": 100.0, "p75_us": 101.0, "min_us": 99.5, "max_us": 101.5, "blocks": 7}
FIELDS = {"this_medians_us", "parent_medians_us", "parent_minus_this_us", "this_spread_us", "parent_spread_us", "spread_us", "off_agrees",
          "off_within_the_parents_own_spread"}


def test_compare_off_agreeing():
    c = H.compare_off([100.0, 101.0], [100.5, 102.5], HANDLE)
    assert set(c) == FIELDS
    assert c["this_medians_us"] == [100.0, 101.0] and c["parent_medians_us"] == [100.5, 102.5]
    assert c["parent_minus_this_us"] == pytest.approx(1.0, abs=1e-12)
    assert (c["this_spread_us"], c["parent_spread_us"], c["spread_us"]) == pytest.approx((1.0, 2.0, 2.0), abs=1e-12)
    assert c["off_agrees"] is True and c["off_within_the_parents_own_spread"] is True


def test_compare_off_disagreeing():
    c = H.compare_off([100.0, 101.0], [103.0, 103.2], HANDLE)
    assert c["parent_minus_this_us"] == pytest.approx(2.6, abs=1e-9)
    assert c["spread_us"] == pytest.approx(2.0, abs=1e-12) and c["off_agrees"] is False
    assert c["parent_spread_us"] == pytest.approx(0.2, abs=1e-9) and c["off_within_the_parents_own_spread"] is False
    # what the four oldest scripts' rule said stays readable from the fields
    assert not abs(c["parent_minus_this_us"]) <= c["this_spread_us"]


# a child that logs where its package comes from, then prints a result, leaves with status 3 or outlives its limit, as CHILD_PLAN says for
# its turn (the number of entries already in the log)
CHILD = r'''
import json, os, sys, time
root = sys.argv[sys.argv.index("--package-root") + 1]
log = os.environ["CHILD_LOG"]
turn = len(open(log).read().splitlines()) if os.path.exists(log) else 0
with open(log, "a") as f:
    f.write(root + "\n")
what = os.environ["CHILD_PLAN"].split(",")[turn]
if what == "fail":
    print("half a line")
    sys.exit(3)
if what == "hang":
    time.sleep(30)
assert sys.argv[1:3] == ["--n", "64"] and sys.argv[-3:] == ["--only-off", "--out", ""]
print("something before the result")
print(json.dumps({"sizes": {"64": {"setups": {"off": {"median_us": 100.0 + turn}}}}}))
'''


@pytest.fixture
def child(tmp_path, monkeypatch):
    script = tmp_path / "child_overhead.py"
    script.write_text(CHILD)
    log = tmp_path / "log.txt"
    monkeypatch.setenv("CHILD_LOG", str(log))

    def plan(p):
        monkeypatch.setenv("CHILD_PLAN", p)
    return str(script), log, plan


def test_fresh_process_returns_the_last_line(child):
    script, log, plan = child
    plan("ok")
    out = H.fresh_process([sys.executable, script, "--n", "64", "--package-root", "somewhere", "--only-off", "--out", ""], 60)
    assert out == {"sizes": {"64": {"setups": {"off": {"median_us": 100.0}}}}}
    assert log.read_text().splitlines() == ["somewhere"]


def test_off_across_builds_alternates_this_and_parent(child, tmp_path):
    script, log, plan = child
    plan("ok,ok,ok,ok")
    parent = str(tmp_path / "parent_tree")
    this, theirs = H.off_across_builds(script, ["--n", 64], parent, 2, lambda run: run["sizes"]["64"]["setups"]["off"]["median_us"], 60)
    assert log.read_text().splitlines() == [H.ROOT, parent, H.ROOT, parent]
    assert this == [100.0, 102.0] and theirs == [101.0, 103.0]


@pytest.mark.parametrize("second, limit", [("fail", 60), ("hang", 1)])
def test_nothing_is_started_after_a_child_that_failed(child, tmp_path, second, limit):
    script, log, plan = child
    plan("ok,%s,ok,ok" % second)
    with pytest.raises(SystemExit):
        H.off_across_builds(script, ["--n", 64], str(tmp_path / "parent_tree"), 2, lambda run: run, limit)
    assert len(log.read_text().splitlines()) == 2


# every flag each script has at the parent commit of the harness (hidden worker flags left out: --help does not print them)
PARENT = ["--parent", "--process-repeats", "--package-root", "--only-off", "--out"]
FLAGS = {
    "auto_component_overhead.py": ["--sizes", "--block", "--warm", "--rounds", "--precondition", "--out"],
    "autoreset_overhead.py": ["--n", "--block", "--rounds", "--out"],
    "bank_autoreset_overhead.py": ["--n", "--bank", "--block", "--rounds", "--out"],
    "column_stats_overhead.py": ["--n", "--block", "--rounds", "--bank", "--bench-steps"] + PARENT,
    "component_maintenance_overhead.py": ["--n", "--block", "--rounds", "--only", "--collect-traces", "--out"],
    "controls_overhead.py": ["--n", "--block", "--rounds", "--bench-steps"] + PARENT,
    "device_noise_overhead.py": ["--n", "--block", "--steps", "--rounds", "--warmup", "--fills", "--no-host", "--out"],
    "diagnostics_carry_overhead.py": ["--parent", "--n", "--rounds", "--blocks", "--block", "--carry-rounds", "--worker-timeout", "--out"],
    "episode_records_overhead.py": ["--n", "--block", "--rounds", "--bank", "--worst-steps", "--bench-steps"] + PARENT,
    "episode_streams_overhead.py": ["--n", "--block", "--rounds", "--profile", "--bank", "--worst-steps", "--stream-block"] + PARENT,
    "event_windows_overhead.py": ["--n", "--block", "--rounds", "--bank", "--bench-steps"] + PARENT,
    "features_overhead.py": ["--n", "--block", "--rounds", "--bank", "--bench-steps"] + PARENT,
    "maintenance_log_overhead.py": ["--n", "--block", "--rounds", "--out"],
    "maintenance_summary_overhead.py": ["--n", "--block", "--rounds", "--busy-span"] + PARENT,
    "minibatch_overhead.py": ["--n", "--rounds", "--calls"] + PARENT,
    "operator_maintenance_overhead.py": ["--n", "--block", "--rounds", "--only", "--collect-traces", "--out"],
    "power_profile_overhead.py": ["--n", "--block", "--horizon", "--steps", "--rounds", "--warmup", "--fills", "--out"],
    "rollout_overhead.py": ["--n", "--rounds", "--calls"] + PARENT,
    "task_overhead.py": ["--n", "--block", "--rounds", "--bank", "--bench-steps"] + PARENT,
    "turbine_maintenance_overhead.py": ["--n", "--block", "--rounds", "--only", "--collect-traces", "--out"],
    "watched_log_overhead.py": ["--sizes", "--rounds", "--block", "--worker-timeout", "--out"],
}


def test_the_table_names_every_overhead_script():
    assert sorted(FLAGS) == sorted(f for f in os.listdir(TOOLS) if f.endswith("_overhead.py"))
    assert len(FLAGS) == 21


@pytest.mark.parametrize("script", sorted(FLAGS))
def test_help_names_every_flag(script):
    p = subprocess.run([sys.executable, os.path.join(TOOLS, script), "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in FLAGS[script]:
        assert re.search(r"(?<![\w-])%s(?![\w-])" % re.escape(flag), p.stdout), (script, flag)
