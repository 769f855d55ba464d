"""CPU: operator-ordered maintenance of the turbine (npb_perform_turbine_maintenance) is declared by include/npb.h, exported by libnpb.so
and bound; a NULL handle is refused; the header's turbine catalog is the binding's and the library's; an unknown name and a handler that
is not offered are refused on the host, each with its own message, before a device is looked for; nuclear_sim_amd.maintlog renders the
fifth record kind and the other four as before.  No compute calls."""
import re

import numpy as np
import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

from turbine_maintenance_golden import ACTIONS, KINDS, NOT_OFFERED, THRUST, UNITS



def _header_catalog():
    """(kind, type string) per X(KIND, ID, "name") line of NPB_TURBINE_ACTIONS in include/npb_maint.h"""
    text = abi.header_text("npb_maint.h")
    body = text[text.index("#define NPB_TURBINE_ACTIONS(X)"):]
    body = body[:body.index("enum {")]
    kinds = {"SYSTEM": "turbine", "BEARING": "bearing", "LUBE": "lubrication", "STAGE": "stage"}
    return text, [(kinds[k], name) for k, name in re.findall(r'X\((\w+),\s*\w+,\s*"(\w+)"\)', body)]


def test_header_declares_the_entry_point_and_the_catalog():
    text, declared = abi.header_text(), set(abi.declared())
    assert {"npb_perform_turbine_maintenance", "npb_turbine_num_actions", "npb_turbine_action_name", "npb_turbine_action_kind",
            "npb_turbine_kind_name", "npb_perform_component_maintenance", "npb_perform_maintenance"} <= declared
    assert abi.define("NPB_VERSION") >= 149
    m = re.search(r"npb_perform_turbine_maintenance\(([^)]*)\)", text[text.index("NPB_API int npb_perform_turbine_maintenance"):])
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["NpbHandle *h", "const int32_t *action", "const int32_t *unit", "uint8_t *success", "void *stream"], args
    maint, catalog = _header_catalog()
    assert re.search(r"NPB_MAINT_EVENT_OPERATOR_TURBINE\s*=\s*4\b", maint) and re.search(r"NPB_MAINT_EVENT_OPERATOR_COMPONENT\s*=\s*3\b", maint)
    assert re.search(r"NPB_MAINT_EVENT_OPERATOR\s*=\s*2\b", maint) and re.search(r"NPB_MAINT_EVENT_COMPLETED\s*=\s*1\b", maint)
    assert abi.define("NPB_TURBINE_NACT", "npb_maint.h") == len(catalog) == len(ACTIONS)
    assert catalog == list(ACTIONS)
    # a catalog of its own: the component catalog keeps its size and its four kinds
    assert abi.define("NPB_COMPONENT_NACT", "npb_maint.h") == 31
    assert re.search(r"NPB_TURBINE_SYSTEM = 0, NPB_TURBINE_BEARING = 1, NPB_TURBINE_LUBE = 2, NPB_TURBINE_STAGE = 3", maint)
    assert "turbine maintenance is not offered" not in text.lower() and "not offered: turbine maintenance" not in text.lower()


def test_host_catalog_is_the_headers_and_the_librarys():
    _maint, catalog = _header_catalog()
    assert list(_lib.TURBINE_ACTIONS) == catalog
    assert _lib.TURBINE_KINDS == KINDS and _lib.TURBINE_UNITS == UNITS and _lib.TURBINE_THRUST_BEARING == THRUST
    L = abi.library()          # load() itself refuses a library whose catalog differs
    n = L.npb_turbine_num_actions()
    assert n == len(catalog)
    assert [(L.npb_turbine_kind_name(L.npb_turbine_action_kind(a)).decode(), L.npb_turbine_action_name(a).decode()) for a in range(n)] == catalog
    assert L.npb_turbine_action_kind(-1) == -1 and L.npb_turbine_action_kind(n) == -1 and L.npb_turbine_action_name(n) is None
    assert L.npb_turbine_kind_name(4) is None and L.npb_turbine_kind_name(-1) is None
    # the catalog is grouped by kind, and a type string occurs once per kind
    assert [k for k, _ in catalog] == sorted((k for k, _ in catalog), key=KINDS.index) and len(set(catalog)) == len(catalog)
    # the component catalog did not move
    assert L.npb_component_num_actions() == 31 and len(_lib.COMPONENT_ACTIONS) == 31


def test_library_exports_and_binding_declares_it():
    abi.check_exported(["npb_perform_turbine_maintenance", "npb_perform_component_maintenance", "npb_perform_maintenance"])
    L = abi.library()
    assert L.npb_version() >= 149
    assert L.npb_perform_turbine_maintenance.argtypes is not None and len(L.npb_perform_turbine_maintenance.argtypes) == 5


def test_null_handle_is_refused():
    abi.check_null_refused([("npb_perform_turbine_maintenance", None, None, None, None, None)])


def test_unknown_and_refused_names_are_told_apart_before_any_device_work():
    """on an object that has no handle, no library and no device behind it"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = object.__new__(BatchedPlantEnv)
    call = BatchedPlantEnv.perform_turbine_maintenance
    with pytest.raises(ValueError, match="unknown turbine maintenance 'polish_the_nameplate'"):
        call(env, "turbine", "polish_the_nameplate")
    with pytest.raises(ValueError, match="unknown turbine component 'condenser'"):
        call(env, "condenser", "routine_maintenance")
    with pytest.raises(ValueError, match="unknown turbine component"):
        call(env, "rotor", 3)
    with pytest.raises(ValueError, match="unknown bearing maintenance 'oil_filter_replacement'"):      # the lubrication system's type on a bearing
        call(env, "bearing", "oil_filter_replacement")
    with pytest.raises(ValueError, match="unknown stage maintenance 'inspection'"):
        call(env, "stage", "inspection", unit=3)
    with pytest.raises(ValueError, match="not offered.*blade_condition_factor"):
        call(env, "stage", "cleaning", unit=3)
    with pytest.raises(ValueError, match="unknown unit"):
        call(env, "bearing", "routine_maintenance", unit="TB-005")
    with pytest.raises(ValueError, match="unknown unit"):
        call(env, "lubrication", "routine_maintenance", unit="TB-001")
    assert set(_lib.TURBINE_ACTIONS_NOT_OFFERED) == set(NOT_OFFERED)
    assert not set(_lib.TURBINE_ACTIONS_NOT_OFFERED) & set(_lib.TURBINE_ACTIONS)
    idx = {_lib.turbine_action_index(k, "routine_maintenance") for k in ("turbine", "bearing", "lubrication")}
    assert len(idx) == 3 and all(_lib.TURBINE_ACTIONS[i][1] == "routine_maintenance" for i in idx)
    assert _lib.turbine_action_index("bearing", "turbine_oil_change") != _lib.turbine_action_index("lubrication", "turbine_oil_change")
    assert _lib.turbine_action_index("stage", 5) == 5
    # the component surface keeps refusing the turbine, as before
    with pytest.raises(ValueError, match="unknown component 'turbine'"):
        BatchedPlantEnv.perform_component_maintenance(env, "turbine", "routine_maintenance")


def test_maintlog_renders_turbine_records_and_leaves_the_others():
    from nuclear_sim_amd import maintlog
    L = abi.library()
    A, P = _lib.MAINT_ACTIONS, _lib.MAINT_PARAMS
    handlers = [int(L.npb_maint_action_has_handler(a)) for a in range(len(A))]
    assert maintlog.OPERATOR_TURBINE == 4 and maintlog.EVENT_TYPES[4] == "operator_turbine_maintenance"
    assert maintlog.EVENT_TYPES[:4] == ("work_order_created", "work_order_completed", "operator_maintenance", "operator_component_maintenance")
    C = list(_lib.COMPONENT_ACTIONS)
    old = np.zeros(5, dtype=maintlog.EVENT_DTYPE)
    old[0] = (10.0, 10.0, 70.0, 1, 3, 1, 1, A.index("oil_top_off"), 0, 3, 0, 0)
    old[1] = (70.0, 10.0, 70.0, 1, 3, 0, 1, A.index("oil_top_off"), 1, 0, 0, 0)
    old[2] = (5.0, 5.0, 5.0, 0, 1, 1 << 5, 3, A.index("cavitation_analysis"), 0, 5, 0, 0)
    old[3] = (70.0, 70.0, 70.0, 1, 0, 0, 0, A.index("bearing_replacement"), maintlog.OPERATOR, 0, 3, 0)
    old[4] = (70.0, 70.0, 70.0, 1, 0, 0, 2, C.index(("steam_generator", "tsp_chemical_cleaning")), maintlog.OPERATOR_COMPONENT, 0, 0, 0)
    T = list(_lib.TURBINE_ACTIONS)
    new = np.zeros(5, dtype=maintlog.EVENT_DTYPE)
    new[0] = (70.0, 70.0, 70.0, 1, 0, 0, 2, T.index(("bearing", "thrust_bearing_adjustment")), 4, 0, 0, 0)
    new[1] = (5.0, 5.0, 5.0, 0, 0, 0, 0, T.index(("turbine", "routine_maintenance")), 4, 0, 0, 0)
    new[2] = (5.0, 5.0, 5.0, 0, 0, 0, 13, T.index(("stage", "overhaul")), 4, 0, 0, 0)
    new[3] = (80.0, 80.0, 80.0, 1, 0, 0, 0, T.index(("lubrication", "turbine_oil_change")), 4, 0, 0, 0)
    new[4] = (80.0, 80.0, 80.0, 1, 0, 0, 8, T.index(("stage", "blade_replacement")), 4, 0, 0, 0)
    before = maintlog.columns(old, A, P, handlers)
    both = maintlog.columns(np.concatenate([new, old]), A, P, handlers)
    sel = both["event_type"] == "operator_turbine_maintenance"
    assert sel.sum() == 5
    assert list(both["plant"][sel]) == [0, 0, 1, 1, 1]
    assert list(both["action_type"][sel]) == ["routine_maintenance", "overhaul", "thrust_bearing_adjustment", "turbine_oil_change", "blade_replacement"]
    assert list(both["component_id"][sel]) == ["SECONDARY-COMP-001-TURB", "LP-6", "TB-003", "TB-LUB-001", "LP-1"]
    assert list(both["work_order_id"][sel]) == [""] * 5 and list(both["priority"][sel]) == [""] * 5 and list(both["work_order_type"][sel]) == [""] * 5
    assert list(both["actual_completion_date"][sel]) == [5.0, 5.0, 70.0, 80.0, 80.0] and list(both["created_date"][sel]) == [5.0, 5.0, 70.0, 80.0, 80.0]
    assert list(both["has_handler"][sel]) == [True] * 5 and list(both["bearing"][sel]) == [""] * 5
    assert both["title"][sel][2] == "Operator: Thrust Bearing Adjustment - TB-003"
    # kinds 0..3 render exactly as without the new records beside them, and keep their relative order
    for k, v in before.items():
        w = both[k][~sel]
        assert len(v) == 5 and all((a == b) or (a != a and b != b) for a, b in zip(v, w)), k
    # within (plant, time): work-order events, then pump orders, then component orders, then turbine orders
    s = maintlog.sort_events(np.concatenate([new, old]))
    assert list(s["kind"]) == [0, 4, 4, 0, 1, 2, 3, 4, 4, 4]


def test_maintlog_ids_are_the_live_references():
    """the ids the log names the turbine's objects by, against what the fixture generator read from the live objects of the data-gen
    runner's plant (ot4) -- and the bearing that is the thrust bearing"""
    from nuclear_sim_amd import maintlog
    from turbine_maintenance_golden import TurbineGolden
    ids = TurbineGolden("ot4_long_run").meta["component_ids"]
    assert [maintlog.turbine_component_id("turbine", 0)] == ids["turbine"] and [maintlog.turbine_component_id("lubrication", 0)] == ids["lubrication"]
    assert [maintlog.turbine_component_id("bearing", k) for k in range(4)] == ids["bearing"]
    assert [maintlog.turbine_component_id("stage", k) for k in range(14)] == ids["stage"]
    assert ids["thrust"] == [ids["bearing"][THRUST]]
    # the two construction constants the lubrication handlers read, and the component the oil-cooler cleaning services
    assert ids["oil_level"] == 100.0 and ids["oil_cooling_effectiveness"] == 1.0 and ids["lubrication_components"].index("oil_coolers") == 4
