"""CPU: the per-plant work-order summary (npb_set_maintenance_summary, nuclear_sim_amd.maintlog.summarize).  The numpy restatement
the device is held to equals, exactly, what the reference's own recorded work orders say (tests/golden/wo_*.json): first creation,
first completion and the counts per (action, pump), with and without a tracking start in the middle of the run; wildcard keys are the
sums and minima of the specific ones; the ABI is declared, exported and bound, and every refusal the library can decide without a
device is made with its message.  No compute calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from golden_util import Golden
from maintenance_summary_ref import WO_FIXTURES, assert_same_tables, feedwater_keys, records_from_orders, reference_summary
from work_order_events import events_from_golden, per_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nuclear_sim_amd", "libnpb.so")
SYMBOLS = ("npb_set_maintenance_summary", "npb_maint_summary_check", "npb_maint_summary_fold", "npb_maint_summary_clear")


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nuclear_sim_amd", "csrc"), "-s"])
    return LIB


_EVENTS = {}


def _events(name):
    """the fixture's events, derived once and never changed"""
    if name not in _EVENTS:
        g = Golden(name)      # (m8 and m10 record their state every other step: their events are taken from the orders themselves)
        ev = events_from_golden(g, _params()) if per_step(g) else records_from_orders(name)
        ev.setflags(write=False)
        _EVENTS[name] = ev
    return _EVENTS[name]


def _params():
    from nuclear_sim_amd import _lib
    return _lib.MAINT_PARAMS


def _one_plant(tables):
    return {k: v[:, 0] for k, v in tables.items()}


@pytest.mark.parametrize("name", WO_FIXTURES)
def test_summarize_equals_the_references_work_orders(name, built_lib):
    """maintlog.summarize over the events the fixture's per-step state implies == the reference's recorded orders, reduced directly:
    from the start, and with a tracking start in the middle of the run (the runner's tracking_start_hours)"""
    from nuclear_sim_amd import maintlog
    g = Golden(name)
    ev = _events(name)
    keys = feedwater_keys()
    assert len(ev) > 0
    mid = float(g.meta.get("dt", 1.0)) * (g.T // 2)
    for since in (0.0, mid):
        want = reference_summary(name, keys, since_minutes=since)
        for what, rec in (("events", ev), ("orders", records_from_orders(name))):
            got = _one_plant(maintlog.summarize(rec, keys, 1, since_minutes=since))
            assert_same_tables(got, want, "%s (%s) since %g" % (name, what, since))
    whole, late = reference_summary(name, keys), reference_summary(name, keys, since_minutes=mid)
    if name.startswith(("m1_", "m2_", "m8_", "z21")):      # the cut is not vacuous: something lies on either side of it
        assert late["n_created"].sum() + late["n_completed"].sum() < whole["n_created"].sum() + whole["n_completed"].sum(), name


def test_m2_has_four_creations_in_one_cell():
    """the case the device's atomics exist for: the four pumps of one plant create oil_top_off at the same clock"""
    from nuclear_sim_amd import maintlog
    ev = _events("m2_oil_top_off_simultaneous")
    s = _one_plant(maintlog.summarize(ev, [("feedwater", "oil_top_off", None)], 1))
    made = ev[ev["kind"] == maintlog.CREATED]
    assert s["n_created"][0] == 4 and len(set(made["time"])) == 1 and s["first_created"][0] == made["time"][0]


@pytest.mark.parametrize("name", ("m2_oil_top_off_simultaneous", "m8_handlers_inspection_overhaul_promotion", "z21_fuzzed_maintenance"))
def test_wildcards_are_sums_and_minima(name, built_lib):
    from nuclear_sim_amd import _lib, maintlog
    ev = np.concatenate([_events(name)] * 3)
    ev["plant"] = np.repeat(np.arange(3), len(_events(name)))
    ev = ev[ev["plant"] != 1]      # a plant without any event keeps "never" and 0
    specific = [("feedwater", a, u) for a in _lib.MAINT_ACTION_NAMES for u in range(4)]
    S = maintlog.summarize(ev, specific, 3)
    W = maintlog.summarize(ev, [("feedwater", None, None)], 3)
    for k in ("n_created", "n_completed"):
        assert np.array_equal(W[k][0], S[k].sum(axis=0)), k
    for k in ("first_created", "first_completed"):
        assert np.array_equal(W[k][0], S[k].min(axis=0)), k
    assert np.all(np.isinf(W["first_created"][0, 1])) and W["n_created"][0, 1] == 0 and W["n_created"][0, 0] > 0
    # per action over the units, and per unit over the actions
    per_action = maintlog.summarize(ev, [("feedwater", a, None) for a in _lib.MAINT_ACTION_NAMES], 3)
    assert np.array_equal(per_action["n_created"], S["n_created"].reshape(18, 4, 3).sum(axis=1))
    assert np.array_equal(per_action["first_completed"], S["first_completed"].reshape(18, 4, 3).min(axis=1))
    per_unit = maintlog.summarize(ev, [("feedwater", None, u) for u in range(4)], 3)
    assert np.array_equal(per_unit["n_completed"], S["n_completed"].reshape(18, 4, 3).sum(axis=0))


def test_kinds_and_catalogs():
    """a record's catalog follows from its kind; operator kinds count as completions and only with operator=True; creation kinds feed
    the created pair"""
    from nuclear_sim_amd import _lib, maintlog
    rec = np.zeros(7, dtype=maintlog.EVENT_DTYPE)
    for k in range(7):
        rec[k] = (10.0 + k, 0.0, 0.0, 0, 0, 0, 1, 1, k, 0, 0, 0)      # kind k at 10 + k minutes, unit 1, action 1 of its catalog
    sg = _lib.COMPONENT_ACTIONS[1]
    tb = _lib.TURBINE_ACTIONS[1]
    keys = [("feedwater", "oil_top_off", 1), ("component", sg, 1), ("turbine", tb, None)]
    work = maintlog.summarize(rec, keys[:2], 1)
    assert work["first_created"][:, 0].tolist() == [10.0, 15.0] and work["first_completed"][:, 0].tolist() == [11.0, 16.0]
    assert work["n_created"][:, 0].tolist() == [1, 1] and work["n_completed"][:, 0].tolist() == [1, 1]
    oper = maintlog.summarize(rec, keys, 1, operator=True)
    assert oper["first_completed"][:, 0].tolist() == [11.0, 13.0, 14.0] and oper["n_completed"][:, 0].tolist() == [2, 2, 1]
    assert oper["n_created"][:, 0].tolist() == [1, 1, 0] and np.isinf(oper["first_created"][2, 0])
    with pytest.raises(ValueError, match="operator=True"):
        _lib.summary_key(("turbine", tb, None))
    with pytest.raises(ValueError, match="polish"):
        _lib.summary_key("polish_the_nameplate")
    with pytest.raises(ValueError, match="catalog"):
        _lib.summary_key(("reactor", None, None))
    with pytest.raises(ValueError, match=r"\(kind, name\)"):
        _lib.summary_key(("component", "routine_maintenance", None))
    assert _lib.summary_key("oil_top_off") == (0, 1, -1, 0b11) and _lib.summary_key(("feedwater", None, 2), operator=True) == (0, -1, 2, 0b111)
    assert _lib.summary_key(("component", ("condenser", "condenser_tube_plugging"), None)) == (1, len(_lib.COMPONENT_ACTIONS), -1, 0b1100000)
    # since_minutes drops exactly the earlier records
    late = maintlog.summarize(rec, keys, 1, since_minutes=11.0, operator=True)
    assert late["n_created"][:, 0].tolist() == [0, 1, 0] and late["first_completed"][0, 0] == 11.0


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "npb.h")).read()
    declared = set(re.findall(r"NPB_API[^;]*?\b(npb_\w+)\s*\(", text))
    assert set(SYMBOLS) <= declared
    assert int(re.search(r"#define NPB_VERSION (\d+)", text).group(1)) == 154
    maint = open(os.path.join(ROOT, "include", "npb_maint.h")).read()
    assert "npb_maint_summary_desc_t" in maint and re.search(r"NPB_MAINT_SUMMARY_MAX_KEYS 16\b", maint)
    assert "+0.0" in maint, "the header must state the precondition of the unsigned minimum"


def test_library_exports_and_binding_declares_them(built_lib):
    lib = ctypes.CDLL(built_lib)
    for s in SYMBOLS:
        assert hasattr(lib, s), "libnpb.so does not export " + s
    assert lib.npb_version() == 154
    from nuclear_sim_amd import _lib
    L = _lib.load()
    assert len(L.npb_set_maintenance_summary.argtypes) == 2 and len(L.npb_maint_summary_clear.argtypes) == 3
    assert ctypes.sizeof(_lib.NpbMaintSummaryDesc) == 16 + 16 * 16 + 6 * 8
    assert ctypes.sizeof(_lib.NpbMaintSummaryKey) == 16


def test_null_handle_is_refused(built_lib):
    from nuclear_sim_amd import _lib
    L = _lib.load()
    d = _lib.NpbMaintSummaryDesc()
    assert L.npb_set_maintenance_summary(None, ctypes.byref(d)) == -1
    assert L.npb_maint_summary_fold(None, None) == -1
    assert L.npb_maint_summary_clear(None, None, None) == -1


def _desc(keys=((0, 1, -1, 3),), consume=0, **over):
    """a descriptor whose tables are made-up, aligned addresses: the check reads no memory"""
    from nuclear_sim_amd import _lib
    d = _lib.NpbMaintSummaryDesc()
    d.n_keys, d.consume, d.since_minutes = len(keys), consume, 0.0
    for j, k in enumerate(keys[:_lib.SUMMARY_MAX_KEYS]):
        d.keys[j].catalog, d.keys[j].action, d.keys[j].unit, d.keys[j].kinds = k
    d.first_created, d.first_completed, d.n_created, d.n_completed, d.folded, d.dropped = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x5004
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_every_refusal_has_its_message(built_lib):
    """npb_maint_summary_check is the check npb_set_maintenance_summary makes (log_capacity < 0 = no log set), without a handle"""
    from nuclear_sim_amd import _lib
    L = _lib.load()

    def why(d, cap=4096, n=64):
        m = L.npb_maint_summary_check(ctypes.byref(d), cap, n)
        return None if m is None else m.decode()
    assert why(_desc()) is None
    assert why(_desc(keys=[(0, a % 18, a % 4, 7) for a in range(16)])) is None
    assert "no maintenance log" in why(_desc(), cap=-1)
    assert "n_keys" in why(_desc(n_keys=0)) and "n_keys" in why(_desc(n_keys=17))
    assert "catalog" in why(_desc(keys=[(3, 0, 0, 1)])) and "catalog" in why(_desc(keys=[(-1, 0, 0, 1)]))
    for cat, nact, kinds in ((0, 18, 1), (1, 32, 0x20), (2, 21, 0x10)):
        assert why(_desc(keys=[(cat, nact - 1, -1, kinds)])) is None
        assert "action" in why(_desc(keys=[(cat, nact, -1, kinds)]))
        assert "action" in why(_desc(keys=[(cat, -2, -1, kinds)]))
    # units: four pumps; three generators, two ejectors, one condenser; four bearings, fourteen stages, one turbine
    sg, cond, ej = _lib.COMPONENT_ACTIONS.index(("steam_generator", "scale_removal")), _lib.COMPONENT_ACTIONS.index(("condenser", "condenser_tube_cleaning")), \
        _lib.COMPONENT_ACTIONS.index(("ejector", "general"))
    brg, stage, tur = _lib.TURBINE_ACTIONS.index(("bearing", "bearing_alignment")), _lib.TURBINE_ACTIONS.index(("stage", "overhaul")), \
        _lib.TURBINE_ACTIONS.index(("turbine", "vibration_analysis"))
    for cat, act, units, kinds in ((0, 1, 4, 1), (0, -1, 4, 1), (1, sg, 3, 0x20), (1, cond, 1, 0x20), (1, ej, 2, 8), (1, 31, 1, 0x20), (1, -1, 3, 0x20),
                                   (2, brg, 4, 0x10), (2, stage, 14, 0x10), (2, tur, 1, 0x10), (2, -1, 14, 0x10)):
        assert why(_desc(keys=[(cat, act, units - 1, kinds)])) is None, (cat, act)
        assert "unit" in why(_desc(keys=[(cat, act, units, kinds)])), (cat, act)
        assert "unit" in why(_desc(keys=[(cat, act, -2, kinds)]))
    assert "kinds" in why(_desc(keys=[(0, 1, -1, 0)]))
    assert "kinds" in why(_desc(keys=[(0, 1, -1, 0x10)])), "a feedwater key with the turbine's kind alone matches nothing"
    assert "kinds" in why(_desc(keys=[(2, 1, -1, 0x07)]))
    for member in ("first_created", "first_completed", "n_created", "n_completed", "folded", "dropped"):
        assert "NULL" in why(_desc(**{member: None})), member
    for member, off in (("first_created", 4), ("first_completed", 4), ("n_created", 2), ("n_completed", 2), ("folded", 2), ("dropped", 1)):
        assert "aligned" in why(_desc(**{member: 0x1000 + off})), member
    assert why(_desc(n_created=0x3004)) is None      # the counts need four bytes only
    assert "consume" in why(_desc(consume=1), cap=63, n=64) and "n_plants" in why(_desc(consume=1), cap=63, n=64)
    assert why(_desc(consume=1), cap=64, n=64) is None and why(_desc(consume=0), cap=8, n=64) is None


def test_env_refuses_bad_keys_before_any_device_work():
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = object.__new__(BatchedPlantEnv)
    with pytest.raises(ValueError, match="polish_the_nameplate"):
        BatchedPlantEnv.enable_maintenance_summary(env, ["polish_the_nameplate"])
    with pytest.raises(ValueError, match="1 to 16"):
        BatchedPlantEnv.enable_maintenance_summary(env, ["oil_top_off"] * 17)
    with pytest.raises(ValueError, match="1 to 16"):
        BatchedPlantEnv.enable_maintenance_summary(env, [])
