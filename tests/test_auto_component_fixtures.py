"""CPU: the fixtures of the automatic maintenance of steam generators and condenser (tests/golden/auto_components/,
tools/make_auto_component_golden.py) are self-consistent -- orders against counters at every step, one completion per check interval,
executed in the order created, every creation at a stamp of its component -- every row of the default table fires in some fixture or is
listed as silent with its reason, every scanned value keeps its distance from its threshold; and the vocabulary around them: the C
default table is the reference's, the entry points are declared, exported and bound, rows are refused by name, the log names the
components.  No compute calls."""
import ctypes
import glob
import json
import os
import re
import subprocess

import numpy as np
import pytest

from golden_util import GOLDEN_DIR, Golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nuclear_sim_amd", "libnpb.so")
DIR = os.path.join(GOLDEN_DIR, "auto_components")
AC = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(DIR, "ac*.npz")))
ENTRY_POINTS = ("npb_set_component_maintenance", "npb_default_component_maintenance_table", "npb_component_maint_num_params",
                "npb_component_maint_param_name", "npb_component_maint_param_kind", "npb_component_maintenance_state_bytes",
                "npb_get_component_maintenance_state", "npb_set_component_maintenance_state")
COMPONENT_IDS = ("SG-0", "SG-1", "SG-2", "SECONDARY-COMP-001-COND")
MARGIN = 1e-5      # what the issue sets: every scanned value at least 1e-5 (relative) from its threshold, at every step


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nuclear_sim_amd", "csrc"), "-s"])
    return LIB


def _load(name):
    z = np.load(os.path.join(DIR, name + ".npz"), allow_pickle=False)
    return Golden("auto_components/" + name), z, json.load(open(os.path.join(DIR, name + ".json")))


def test_the_six_runs_are_there():
    assert len(AC) >= 6 and AC[0] == "ac1_shared_queue", AC


@pytest.mark.parametrize("name", AC)
def test_orders_counters_and_queue(name):
    g, z, side = _load(name)
    orders = side["orders"]
    dt, interval = float(g.meta["dt"]), side["check_interval_minutes"]
    assert [o["work_order_id"] for o in orders] == ["WO-%06d" % (k + 1) for k in range(len(orders))]      # one counter, no gaps
    done = [o for o in orders if o["completed"] is not None]
    assert side["counters"] == {"work_orders_created": len(orders), "maintenance_actions_performed": len(done)}
    # the counters of every recorded state are the orders created / completed by then
    labels = [c[2] for c in g.cols]
    created_col, performed_col = labels.index("maint.work_orders_created"), labels.index("maint.maintenance_actions_performed")
    for j, s in enumerate(g.state_steps):
        clock = int(s) * dt
        assert g.state[j, created_col] == sum(o["created"] <= clock for o in orders), (name, s)
        assert g.state[j, performed_col] == sum(o["completed"] <= clock for o in done), (name, s)
    # one completion per check, in the order created, none before its planned start; an order left open is younger than every completed one
    times = [o["completed"] for o in done]
    assert all(b - a >= interval for a, b in zip(times, times[1:])), times
    assert [o["work_order_id"] for o in sorted(done, key=lambda o: o["completed"])] == [o["work_order_id"] for o in done]
    # ... every order succeeds but condenser_tube_plugging, whose handler raises in the reference: completed and counted all the same
    assert all(o["completed"] >= o["planned"] >= o["created"] and o["success"] is (o["action"] != "condenser_tube_plugging") for o in done)
    still_open = [o for o in orders if o["completed"] is None]
    assert all(o["work_order_id"] > done[-1]["work_order_id"] for o in still_open)
    if name == "ac7_tube_leak":
        assert [(o["component_id"], o["action"], o["success"]) for o in done][0] == ("SECONDARY-COMP-001-COND", "condenser_tube_plugging", False)
    # every order on a scanned component was created at a stamp of one of its rows; stamps only ever move to the clock
    stamps = z["stamps"]
    assert stamps.shape == (g.T + 1, 12) and (stamps[0] == -1.0).all()
    for t in range(g.T):
        moved = stamps[t + 1] != stamps[t]
        assert (stamps[t + 1][moved] == (t + 1) * dt).all()
    for o in orders:
        if o["component_id"] in COMPONENT_IDS:
            c = COMPONENT_IDS.index(o["component_id"])
            assert (stamps[:, 3 * c:3 * c + 3] == o["created"]).any(), o
    assert not g.done.any()


def test_pumps_and_components_share_the_queue():
    """the probe run: a pump's order is numbered behind five component orders; in the edited-table run it waits its turn"""
    _g, _z, side = _load("ac1_shared_queue")
    assert [(o["component_id"], o["action"], o["created"], o["completed"]) for o in side["orders"]] == [
        ("SG-0", "tsp_chemical_cleaning", 5.0, 20.0), ("SG-2", "tsp_chemical_cleaning", 5.0, 35.0),
        ("SECONDARY-COMP-001-COND", "condenser_tube_cleaning", 5.0, 50.0), ("SG-0", "scale_removal", 10.0, 65.0),
        ("SG-1", "scale_removal", 10.0, 80.0), ("FWP-1", "oil_top_off", 140.0, 155.0)]
    _g, _z, side = _load("ac6_edited_table")
    pump = [o for o in side["orders"] if o["component_id"].startswith("FWP-")]
    assert len(pump) == 1 and pump[0]["completed"] - pump[0]["planned"] > side["check_interval_minutes"]      # held up by component orders before it


def test_every_default_row_fires_or_is_listed_silent():
    from nuclear_sim_amd import _lib
    silent = json.load(open(os.path.join(DIR, "silent_rows.json")))["default_table_rows_silent"]
    fired = set()
    for name in AC:
        g, z, side = _load(name)
        if g.meta.get("table_edits"):
            continue
        for c in range(4):
            rows = [n for k, n in _lib.CMAINT_PARAMS if k == ("condenser" if c == 3 else "steam_generator")]
            for r, n in enumerate(rows):
                if (z["stamps"][:, 3 * c + r] >= 0).any():
                    fired.add("%s:%s" % ("condenser" if c == 3 else "steam_generator", n))
    for kind, n in _lib.CMAINT_PARAMS:
        key = "%s:%s" % (kind, n)
        assert key in fired or (key in silent and len(silent[key]) > 40), key
    assert not fired & set(silent)
    # ... and the silent row does fire under an edited table, so the device's scan of it is exercised
    _g, z, _side = _load("ac6_edited_table")
    assert (z["stamps"][:, [2, 5, 8]] >= 0).any()
    # every row of these components that resolves on the reference is scanned on the device
    for name in AC:
        assert _load(name)[2]["silent"] == {}
    # the turbine's rows, which the device does not scan: tried on the live reference with the stages' carried state at its worst, silent
    probe = json.load(open(os.path.join(DIR, "silent_rows.json")))["turbine_efficiency_probe"]
    assert len(probe["lowest_efficiency_scanned"]) == 15 and min(probe["lowest_efficiency_scanned"].values()) >= 0.7 > probe["threshold"]
    assert probe["rows_fired"] == [] and probe["orders_on_turbine_components"] == []


def test_edited_table_runs_pin_the_orchestrator_paths():
    """ac8: the three rows of SG-0 stamped in one step (t = 65) and no order on SG-0 then -- promoted to tube_bundle_overhaul, which is no
    action type -- while two rows an hour later give one; ac9: a row naming a handler that is no action type is stamped and orders nothing"""
    _g, z, side = _load("ac8_overhaul_promotion")
    assert (z["stamps"][13, 0:3] == 65.0).all() and not [o for o in side["orders"] if o["component_id"] == "SG-0" and o["created"] == 65.0]
    assert [o["action"] for o in side["orders"] if o["component_id"] == "SG-0" and o["created"] == 125.0] == ["tsp_mechanical_cleaning"]
    _g, z, side = _load("ac9_action_is_no_type")
    assert (z["stamps"][:, 4] == 10.0).any() and side["orders"] == [] and dict(side["table"]["steam_generator"])["tube_wall_temperature"]["action"] == "primary_scale_cleaning"


@pytest.mark.parametrize("name", AC)
def test_scanned_values_keep_their_distance(name):
    _g, z, side = _load(name)
    thr, scanned = z["thresholds"], z["scanned"]
    used = ~np.isnan(thr)
    assert used.sum() == 11 and not np.isnan(scanned[:, used]).any()
    d = np.abs(scanned[:, used] - thr[None, used]) / np.abs(thr[None, used])
    assert d.min() >= MARGIN, (name, d.min())
    assert side["margin"] == MARGIN


def test_header_declares_and_library_exports(built_lib):
    text = open(os.path.join(ROOT, "include", "npb.h")).read()
    declared = set(re.findall(r"NPB_API[^;]*?\b(npb_\w+)\s*\(", text))
    lib = ctypes.CDLL(built_lib)
    for s in ENTRY_POINTS:
        assert s in declared and hasattr(lib, s), s
    assert int(re.search(r"#define NPB_VERSION (\d+)", text).group(1)) >= 150 and lib.npb_version() >= 150
    from nuclear_sim_amd import _lib
    L = _lib.load()
    assert L.npb_set_component_maintenance.argtypes is not None
    assert L.npb_set_component_maintenance(None, None) == -1 and L.npb_get_component_maintenance_state(None, None, None) == -1
    assert L.npb_component_maintenance_state_bytes(None) == 0


def test_default_table_is_the_references(built_lib):
    """npb_default_component_maintenance_table against the table the live reference ran ac1 with"""
    from nuclear_sim_amd import _lib
    L = _lib.load()
    mine = _lib.NpbComponentMaintTable()
    L.npb_default_component_maintenance_table(ctypes.byref(mine))
    side = _load("ac1_shared_queue")[2]
    theirs = _lib.component_maint_table_from_thresholds({k: dict((n, c) for n, c in side["table"][k]) for k in ("steam_generator", "condenser")})
    for field, _t in _lib.NpbComponentMaintTable._fields_:
        assert list(getattr(mine, field)) == list(getattr(theirs, field)), field
    assert all(r >= 0 for r in mine.rank)


def test_rows_are_refused_by_name():
    from nuclear_sim_amd import _lib
    row = {"threshold": 1.0, "action": "scale_removal"}
    with pytest.raises(_lib.NpbError, match="unknown steam_generator threshold parameter 'bogus'"):
        _lib.component_maint_table_from_thresholds({"steam_generator": {"bogus": row}})
    with pytest.raises(_lib.NpbError, match="not in the component catalog"):
        _lib.component_maint_table_from_thresholds({"condenser": {"fouling_resistance": row}})      # a generator's action on the condenser
    with pytest.raises(_lib.NpbError, match="not in the component catalog"):
        _lib.component_maint_table_from_thresholds({"steam_generator": {"steam_quality": dict(row, action="condenser_tube_plugging")}})
    with pytest.raises(_lib.NpbError, match="unknown comparison"):
        _lib.component_maint_table_from_thresholds({"steam_generator": {"steam_quality": dict(row, comparison="about")}})
    with pytest.raises(_lib.NpbError, match="covers"):
        _lib.component_maint_table_from_thresholds({"ejector": {}})
    with pytest.raises(_lib.NpbError, match="not scanned on the device.*max\\(0.7"):      # refused with the measured reason, not dropped
        _lib.component_maint_table_from_thresholds({"turbine": {"efficiency": dict(row, action="efficiency_analysis")}})
    # rows the reference never resolves are dropped; tube_leak_rate is scanned, with the action from behind the catalog
    t = _lib.component_maint_table_from_thresholds({"steam_generator": {"efficiency": row, "steam_quality": row},
                                                    "condenser": {"tube_leak_rate": dict(row, action="condenser_tube_plugging"), "vacuum_level": row}})
    assert list(t.rank) == [-1, -1, 1, -1, 0] and t.action[4] == len(_lib.COMPONENT_ACTIONS)


def test_log_names_component_orders():
    from nuclear_sim_amd import _lib, maintlog
    rec = np.zeros(3, dtype=maintlog.EVENT_DTYPE)
    rec["kind"] = [maintlog.COMPONENT_CREATED, maintlog.COMPONENT_COMPLETED, maintlog.COMPONENT_CREATED]
    rec["action"] = [_lib.COMPONENT_ACTIONS.index(("steam_generator", "scale_removal"))] * 2 + [_lib.COMPONENT_ACTIONS.index(("condenser", "condenser_tube_cleaning"))]
    rec["pump"] = [2, 2, 0]; rec["bearing"] = [0, 0, 2]; rec["order"] = [4, 4, 5]; rec["priority"] = [3, 3, 5]; rec["trigger"] = [2, 0, 1]
    rec["time"] = [10.0, 65.0, 10.0]; rec["created"] = 10.0; rec["planned_start"] = 10.0; rec["reserved"] = [0, 1, 0]
    cols = maintlog.columns(rec, _lib.MAINT_ACTION_NAMES, ["p%d" % k for k in range(16)], [1] * 18, naming="composed", with_success=True)
    by_event = {(cols["work_order_id"][j], cols["event_type"][j]): j for j in range(3)}
    j = by_event[("WO-000004", "work_order_created")]
    assert (cols["component_id"][j], cols["action_type"][j], cols["priority"][j], cols["trigger_parameters"][j], cols["work_order_type"][j]) == (
        "SG-2", "scale_removal", "HIGH", "tube_wall_temperature", "corrective")
    j = by_event[("WO-000004", "work_order_completed")]
    assert cols["actual_completion_date"][j] == 65.0 and cols["success"][j] and cols["priority"][j] == "HIGH"
    j = by_event[("WO-000005", "work_order_created")]
    assert (cols["component_id"][j], cols["work_order_type"][j], cols["trigger_parameters"][j]) == ("SECONDARY-COMP-001-COND", "emergency", "fouling_resistance")
    assert maintlog.columns(rec, _lib.MAINT_ACTION_NAMES, ["p%d" % k for k in range(16)], [1] * 18)["component_id"][j] == "SECONDARY-001-COND"
