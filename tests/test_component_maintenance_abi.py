"""CPU: operator-ordered maintenance of steam generators and condenser (npb_perform_component_maintenance) is declared by include/npb.h,
exported by libnpb.so and bound; a NULL handle is refused; the header's component catalog is the binding's and the library's; an unknown
name and a handler that is not offered are refused on the host, each with its own message, before a device is looked for;
nuclear_sim_amd.maintlog renders the fourth record kind and the other three as before.  No compute calls."""
import re

import numpy as np
import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

from component_maintenance_golden import ACTIONS, KINDS, UNITS



def _header_catalog():
    """(kind, type string) per X(KIND, ID, "name") line of NPB_COMPONENT_ACTIONS in include/npb_maint.h"""
    text = abi.header_text("npb_maint.h")
    body = text[text.index("#define NPB_COMPONENT_ACTIONS(X)"):]
    body = body[:body.index("enum {")]
    kinds = {"SG": "steam_generator", "SGSYS": "steam_generator_system", "COND": "condenser", "EJECTOR": "ejector"}
    return text, [(kinds[k], name) for k, name in re.findall(r'X\((\w+),\s*\w+,\s*"(\w+)"\)', body)]


def test_header_declares_the_entry_point_and_the_catalog():
    text, declared = abi.header_text(), set(abi.declared())
    assert {"npb_perform_component_maintenance", "npb_component_num_actions", "npb_component_action_name", "npb_component_action_kind",
            "npb_perform_maintenance"} <= declared
    assert abi.define("NPB_VERSION") >= 148
    m = re.search(r"npb_perform_component_maintenance\(([^)]*)\)", text[text.index("NPB_API int npb_perform_component_maintenance"):])
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["NpbHandle *h", "const int32_t *action", "const int32_t *unit", "const int32_t *option", "const double *amount",
                    "uint8_t *success", "void *stream"], args
    maint, catalog = _header_catalog()
    assert re.search(r"NPB_MAINT_EVENT_OPERATOR_COMPONENT\s*=\s*3\b", maint) and re.search(r"NPB_MAINT_EVENT_OPERATOR\s*=\s*2\b", maint)
    assert abi.define("NPB_COMPONENT_NACT", "npb_maint.h") == len(catalog) == len(ACTIONS)
    assert catalog == list(ACTIONS)


def test_host_catalog_is_the_headers_and_the_librarys():
    _maint, catalog = _header_catalog()
    assert list(_lib.COMPONENT_ACTIONS) == catalog
    assert _lib.COMPONENT_KINDS == KINDS and _lib.COMPONENT_UNITS == UNITS
    L = abi.library()          # load() itself refuses a library whose catalog differs
    n = L.npb_component_num_actions()
    assert n == len(catalog)
    assert [(L.npb_component_kind_name(L.npb_component_action_kind(a)).decode(), L.npb_component_action_name(a).decode()) for a in range(n)] == catalog
    assert L.npb_component_action_kind(-1) == -1 and L.npb_component_action_kind(n) == -1 and L.npb_component_action_name(n) is None
    assert L.npb_component_kind_name(4) is None
    # the catalog is grouped by kind, and a type string occurs once per kind
    assert [k for k, _ in catalog] == sorted((k for k, _ in catalog), key=KINDS.index) and len(set(catalog)) == len(catalog)


def test_library_exports_and_binding_declares_it():
    abi.check_exported(["npb_perform_component_maintenance", "npb_perform_maintenance"])
    L = abi.library()
    assert L.npb_version() >= 148
    assert L.npb_perform_component_maintenance.argtypes is not None and len(L.npb_perform_component_maintenance.argtypes) == 7
    assert len(L.npb_perform_maintenance.argtypes) == 7


def test_null_handle_is_refused():
    abi.check_null_refused([("npb_perform_component_maintenance", None, None, None, None, None, None, None)])


def test_unknown_and_refused_names_are_told_apart_before_any_device_work():
    """on an object that has no handle, no library and no device behind it"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = object.__new__(BatchedPlantEnv)
    call = BatchedPlantEnv.perform_component_maintenance
    with pytest.raises(ValueError, match="unknown steam_generator maintenance 'polish_the_nameplate'"):
        call(env, "steam_generator", "polish_the_nameplate")
    with pytest.raises(ValueError, match="unknown component 'turbine'"):
        call(env, "turbine", "routine_maintenance")
    with pytest.raises(ValueError, match="unknown component"):
        call(env, "turbine", 3)
    with pytest.raises(ValueError, match="unknown condenser maintenance 'tsp_chemical_cleaning'"):      # a generator's type on the condenser
        call(env, "condenser", "tsp_chemical_cleaning")
    with pytest.raises(ValueError, match="not offered.*tube_count"):
        call(env, "condenser", "condenser_tube_plugging", tubes_to_plug=25)
    with pytest.raises(ValueError, match="not offered.*operating_years"):
        call(env, "steam_generator", "eddy_current_testing")
    with pytest.raises(ValueError, match="unknown unit"):
        call(env, "ejector", "vacuum_ejector_cleaning", unit="SJE-003")
    assert set(_lib.COMPONENT_ACTIONS_NOT_OFFERED) == {("condenser", "condenser_tube_plugging"), ("steam_generator", "eddy_current_testing")}
    assert not set(_lib.COMPONENT_ACTIONS_NOT_OFFERED) & set(_lib.COMPONENT_ACTIONS)
    assert _lib.component_action_index("steam_generator", "routine_maintenance") != _lib.component_action_index("ejector", "routine_maintenance")
    assert _lib.COMPONENT_ACTIONS[_lib.component_action_index("steam_generator_system", "routine_maintenance")][0] == "steam_generator_system"
    assert _lib.component_action_index("condenser", 5) == 5
    assert [_lib.cleaning_type_index(c) for c in (None, "chemical", "mechanical", "hydroblast", "replacement", "brush", 2)] == [0, 1, 2, 3, 4, 5, 2]


def test_maintlog_renders_component_records_and_leaves_the_others():
    from nuclear_sim_amd import maintlog
    L = abi.library()
    A, P = _lib.MAINT_ACTIONS, _lib.MAINT_PARAMS
    handlers = [int(L.npb_maint_action_has_handler(a)) for a in range(len(A))]
    assert maintlog.OPERATOR_COMPONENT == 3 and maintlog.EVENT_TYPES[3] == "operator_component_maintenance"
    assert maintlog.EVENT_TYPES[:3] == ("work_order_created", "work_order_completed", "operator_maintenance")
    old = np.zeros(4, dtype=maintlog.EVENT_DTYPE)
    old[0] = (10.0, 10.0, 70.0, 1, 3, 1, 1, A.index("oil_top_off"), 0, 3, 0, 0)
    old[1] = (70.0, 10.0, 70.0, 1, 3, 0, 1, A.index("oil_top_off"), 1, 0, 0, 0)
    old[2] = (5.0, 5.0, 5.0, 0, 1, 1 << 5, 3, A.index("cavitation_analysis"), 0, 5, 0, 0)
    old[3] = (70.0, 70.0, 70.0, 1, 0, 0, 0, A.index("bearing_replacement"), maintlog.OPERATOR, 0, 3, 0)
    C = list(_lib.COMPONENT_ACTIONS)
    new = np.zeros(4, dtype=maintlog.EVENT_DTYPE)
    new[0] = (70.0, 70.0, 70.0, 1, 0, 0, 2, C.index(("steam_generator", "tsp_chemical_cleaning")), 3, 0, 0, 0)
    new[1] = (5.0, 5.0, 5.0, 0, 0, 0, 0, C.index(("condenser", "condenser_tube_cleaning")), 3, 0, 0, 0)
    new[2] = (5.0, 5.0, 5.0, 0, 0, 0, 1, C.index(("ejector", "routine_maintenance")), 3, 0, 0, 0)
    new[3] = (80.0, 80.0, 80.0, 1, 0, 0, 0, C.index(("steam_generator_system", "routine_maintenance")), 3, 0, 0, 0)
    before = maintlog.columns(old, A, P, handlers)
    both = maintlog.columns(np.concatenate([new, old]), A, P, handlers)
    sel = both["event_type"] == "operator_component_maintenance"
    assert sel.sum() == 4
    assert list(both["plant"][sel]) == [0, 0, 1, 1]
    assert list(both["action_type"][sel]) == ["condenser_tube_cleaning", "routine_maintenance", "tsp_chemical_cleaning", "routine_maintenance"]
    assert list(both["component_id"][sel]) == ["CONDENSER", "SJE-002", "SG-2", "SG-SYSTEM"]
    assert list(both["work_order_id"][sel]) == [""] * 4 and list(both["priority"][sel]) == [""] * 4 and list(both["work_order_type"][sel]) == [""] * 4
    assert list(both["actual_completion_date"][sel]) == [5.0, 5.0, 70.0, 80.0] and list(both["created_date"][sel]) == [5.0, 5.0, 70.0, 80.0]
    assert list(both["has_handler"][sel]) == [True] * 4 and list(both["bearing"][sel]) == [""] * 4
    assert both["title"][sel][2] == "Operator: Tsp Chemical Cleaning - SG-2"
    # kinds 0..2 render exactly as without the new records beside them, and keep their relative order
    for k, v in before.items():
        w = both[k][~sel]
        assert len(v) == 4 and all((a == b) or (a != a and b != b) for a, b in zip(v, w)), k
    # within (plant, time): work-order events, then pump orders, then component orders
    s = maintlog.sort_events(np.concatenate([new, old]))
    assert list(s["kind"]) == [0, 3, 3, 0, 1, 2, 3, 3]
