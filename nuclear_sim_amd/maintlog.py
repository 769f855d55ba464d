"""The maintenance event log as the reference's data-gen runner exports it.

``npb_set_maintenance_log`` (include/npb.h) has the automatic maintenance append one ``npb_maint_event_t`` record (include/npb_maint.h)
per work order it creates or completes, and ``npb_perform_maintenance`` / ``npb_perform_component_maintenance`` /
``npb_perform_turbine_maintenance`` one per action a caller ordered.  This module turns drained
records into columns named as the reference's ``MaintenanceScenarioRunner.export_data`` writes its ``*_work_orders.csv`` / ``*_maintenance_actions.csv``
(maintenance_scenario_runner.py:1071-1231) and as ``WorkOrderManager`` holds the orders (work_orders.py).  Host code only.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

# include/npb_maint.h npb_maint_event_t, 40 bytes
EVENT_DTYPE = np.dtype([("time", "<f8"), ("created", "<f8"), ("planned_start", "<f8"), ("plant", "<i4"), ("order", "<i4"),
                        ("trigger", "<u2"), ("pump", "u1"), ("action", "u1"), ("kind", "u1"), ("priority", "u1"), ("bearing", "u1"),
                        ("reserved", "u1")])
CREATED, COMPLETED, OPERATOR, OPERATOR_COMPONENT, OPERATOR_TURBINE, COMPONENT_CREATED, COMPONENT_COMPLETED = 0, 1, 2, 3, 4, 5, 6    # NPB_MAINT_EVENT_*
# OPERATOR: an action ordered through npb_perform_maintenance (BatchedPlantEnv.perform_maintenance) and carried out at once: no work
# order (order 0, id ""), created = planned start = time = the plant's clock at the call
# OPERATOR_COMPONENT: the same through npb_perform_component_maintenance (BatchedPlantEnv.perform_component_maintenance): ``action`` is an
# index of the COMPONENT catalog (include/npb_maint.h NPB_COMPONENT_ACTIONS, _lib.COMPONENT_ACTIONS), the ``pump`` byte the unit
# (generator 0..2, ejector 0..1; 0 for the system and the condenser)
# OPERATOR_TURBINE: the same through npb_perform_turbine_maintenance (BatchedPlantEnv.perform_turbine_maintenance): ``action`` is an index of
# the TURBINE catalog (NPB_TURBINE_ACTIONS, _lib.TURBINE_ACTIONS), the ``pump`` byte the unit (bearing 0..3, stage 0..13; 0 for the turbine and
# the lubrication system)
# COMPONENT_CREATED / COMPONENT_COMPLETED: a work order of the automatic maintenance of a steam generator or the condenser
# (npb_set_component_maintenance): ``action`` an index of the COMPONENT catalog, the ``pump`` byte the unit, the ``bearing`` byte the component
# kind (0 steam generator, 2 condenser), ``priority`` on both records, ``trigger`` bit r = row r of the component (its parameters in
# _lib.CMAINT_PARAMS order), the ``reserved`` byte of a completion = the result's success; ``order`` is the reference's number: pumps and
# components count from one counter
EVENT_TYPES = ("work_order_created", "work_order_completed", "operator_maintenance", "operator_component_maintenance",
               "operator_turbine_maintenance", "work_order_created", "work_order_completed")
# the reference's id of the condenser under each naming of the plant's providers (BatchedPlantEnv.log_naming: "composed" = the data-gen
# composer's configuration, "default" = a default-constructed simulator's; nuclear_sim_amd/statelog.py log_column_name)
CONDENSER_IDS = {"composed": "SECONDARY-COMP-001-COND", "default": "SECONDARY-001-COND"}
# the reference's ids of the turbine's objects as the data-gen runner's plant names them: the turbine's config.system_id, the keys of
# rotor_dynamics.bearings and stage_system.stages, the lubrication system's config.system_id (tests/golden/operator_turbine/ot4_long_run.npz
# records them from the live objects)
TURBINE_ID, TURBINE_LUBRICATION_ID = "SECONDARY-COMP-001-TURB", "TB-LUB-001"
TURBINE_BEARING_IDS = ("TB-001", "TB-002", "TB-003", "TB-004")
TURBINE_STAGE_IDS = tuple(["HP-%d" % k for k in range(1, 9)] + ["LP-%d" % k for k in range(1, 7)])
PRIORITY_NAMES = {1: "LOW", 2: "MEDIUM", 3: "HIGH", 4: "CRITICAL", 5: "EMERGENCY"}    # work_orders.py Priority
BEARING_NAMES = {1: "motor", 2: "pump", 3: "thrust"}       # NPB_BEARING_*: the threshold's component_id


def work_order_type(action: str, priority: Optional[int]) -> str:
    """AutoMaintenanceSystem._create_automatic_work_order's rule (auto_maintenance.py:380-395)"""
    if priority == 5:
        return "emergency"
    if "inspection" in action or "analysis" in action:
        return "inspection"
    if "cleaning" in action or "flush" in action:
        return "cleaning"
    return "corrective"


def work_order_title(action: str, component_id: str) -> str:
    """the order's title (auto_maintenance.py:398)"""
    return "Auto: %s - %s" % (action.replace("_", " ").title(), component_id)


def sort_events(rec: np.ndarray) -> np.ndarray:
    """by (plant, time, completion before creation before operator action, pump): the device appends in no particular order.  An
    operator action follows the step whose clock it carries, so it sorts behind that step's work-order events; two operator actions of
    one plant on one pump at one time keep the order they are given in (the device's)."""
    rec = np.asarray(rec, dtype=EVENT_DTYPE)
    rank = np.where((rec["kind"] == COMPLETED) | (rec["kind"] == COMPONENT_COMPLETED), 0, np.where(rec["kind"] == OPERATOR, 2, np.where(rec["kind"] == OPERATOR_COMPONENT, 3,
                                                                                             np.where(rec["kind"] == OPERATOR_TURBINE, 4, 1))))
    return rec[np.lexsort((rec["pump"], rank, rec["time"], rec["plant"]))]


def component_id(kind: str, unit: int) -> str:
    """the reference's name of the object an operator component action was ordered on (SG-<i> as enhanced_physics.py:1099 numbers the
    generators, the ejectors' own ids vacuum_system.py; the two single objects by their role)"""
    if kind == "steam_generator":
        return "SG-%d" % unit
    if kind == "ejector":
        return ("SJE-001", "SJE-002")[unit] if 0 <= unit < 2 else "SJE-?"
    return {"steam_generator_system": "SG-SYSTEM", "condenser": "CONDENSER"}[kind]


def turbine_component_id(kind: str, unit: int) -> str:
    """the reference's id of the object an operator turbine action was ordered on"""
    if kind == "bearing":
        return TURBINE_BEARING_IDS[unit] if 0 <= unit < len(TURBINE_BEARING_IDS) else "TB-?"
    if kind == "stage":
        return TURBINE_STAGE_IDS[unit] if 0 <= unit < len(TURBINE_STAGE_IDS) else "STAGE-?"
    return {"turbine": TURBINE_ID, "lubrication": TURBINE_LUBRICATION_ID}[kind]


def auto_component_id(kind: int, unit: int, naming: str = "default") -> str:
    """the reference's id of the object an automatic component order names: SG-<i>, or the condenser's id under ``naming``"""
    return "SG-%d" % unit if kind == 0 else CONDENSER_IDS[naming]


def columns(rec: np.ndarray, actions: Sequence[str], params: Sequence[str], handlers: Sequence[int], naming: str = "default",
            with_success: bool = False) -> Dict[str, np.ndarray]:
    """Drained records -> columns, sorted by ``sort_events``.  ``actions`` / ``params`` / ``handlers``: the catalogs of
    include/npb_maint.h (``_lib.MAINT_ACTIONS``, ``_lib.MAINT_PARAMS``, ``npb_maint_action_has_handler``).  A completion takes its
    priority from its creation record when that record is among ``rec``, else it has none ("").  An operator action
    (``event_type`` "operator_maintenance", "operator_component_maintenance", "operator_turbine_maintenance") has no work order: its id,
    priority and work-order type are "", its dates the time of the call; a component action is named from the component catalog and its
    object (``component_id``), a turbine action from the turbine catalog (``turbine_component_id``)."""
    from ._lib import CMAINT_AUTO_ACTIONS, COMPONENT_ACTIONS, TURBINE_ACTIONS
    rec = sort_events(rec)
    n = len(rec)
    kind = rec["kind"].astype(np.int64)
    auto_comp = (kind == COMPONENT_CREATED) | (kind == COMPONENT_COMPLETED)      # orders on a generator or the condenser: named from the COMPONENT catalog
    created = (kind == CREATED) | (kind == COMPONENT_CREATED)
    prio_of = {(int(p), int(o)): int(q) for p, o, q in zip(rec["plant"][created], rec["order"][created], rec["priority"][created])}
    operator = (kind == OPERATOR) | (kind == OPERATOR_COMPONENT) | (kind == OPERATOR_TURBINE)
    prio = np.array([int(q) if k in (CREATED, COMPONENT_CREATED, COMPONENT_COMPLETED) else (0 if op else prio_of.get((int(p), int(o)), 0))
                     for k, op, p, o, q in zip(kind, operator, rec["plant"], rec["order"], rec["priority"])], dtype=np.int64)
    auto_names = {v: k[1] for k, v in CMAINT_AUTO_ACTIONS.items()}      # an automatic order's action from behind the catalog
    action = [auto_names[int(a)] if int(a) in auto_names and k in (COMPONENT_CREATED, COMPONENT_COMPLETED) else
              COMPONENT_ACTIONS[int(a)][1] if k in (OPERATOR_COMPONENT, COMPONENT_CREATED, COMPONENT_COMPLETED) else TURBINE_ACTIONS[int(a)][1] if k == OPERATOR_TURBINE else actions[int(a)]
              for a, k in zip(rec["action"], kind)]
    component = [auto_component_id(int(b), int(u), naming) if k in (COMPONENT_CREATED, COMPONENT_COMPLETED) else
                 component_id(COMPONENT_ACTIONS[int(a)][0], int(u)) if k == OPERATOR_COMPONENT else
                 turbine_component_id(TURBINE_ACTIONS[int(a)][0], int(u)) if k == OPERATOR_TURBINE else "FWP-%d" % (int(u) + 1)
                 for u, a, k, b in zip(rec["pump"], rec["action"], kind, rec["bearing"])]
    time = rec["time"].astype(np.float64)
    out = {
        "plant": rec["plant"].astype(np.int64),
        "pump": rec["pump"].astype(np.int64),
        "action_type": np.array(action, dtype=object),
        "event_type": np.array([EVENT_TYPES[k] for k in kind], dtype=object),
        "timestamp_minutes": time,
        "timestamp_hours": time / 60.0,
        "work_order_id": np.array(["WO-%06d" % int(o) if not op else "" for o, op in zip(rec["order"], operator)], dtype=object),
        "component_id": np.array(component, dtype=object),
        "priority": np.array([PRIORITY_NAMES.get(int(q), "") for q in prio], dtype=object),
        "work_order_type": np.array([work_order_type(a, int(q) or None) if not op else "" for a, q, op in zip(action, prio, operator)], dtype=object),
        "title": np.array([work_order_title(a, c) if not op else "Operator: %s - %s" % (a.replace("_", " ").title(), c)
                           for a, c, op in zip(action, component, operator)], dtype=object),
        "created_date": rec["created"].astype(np.float64),
        "planned_start_date": rec["planned_start"].astype(np.float64),
        "actual_completion_date": np.where((kind == COMPLETED) | (kind == COMPONENT_COMPLETED) | operator, time, np.nan),
        "bearing": np.array([BEARING_NAMES.get(int(b), "") if not ac else "" for b, ac in zip(rec["bearing"], auto_comp)], dtype=object),
        "trigger_parameters": np.array([";".join(_component_rows(int(b))[q] for q in range(3) if (int(m) >> q) & 1 and q < len(_component_rows(int(b)))) if ac else
                                        ";".join(params[q] for q in range(len(params)) if (int(m) >> q) & 1)
                                        for m, ac, b in zip(rec["trigger"], auto_comp, rec["bearing"])], dtype=object),
        "has_handler": np.array([k in (OPERATOR_COMPONENT, OPERATOR_TURBINE, COMPONENT_CREATED, COMPONENT_COMPLETED) or bool(handlers[int(a)])
                                 for a, k in zip(rec["action"], kind)], dtype=bool) if n else np.zeros(0, dtype=bool),
    }
    if with_success:      # (only where component orders can occur, so that a log of the pumps alone keeps the columns it had)
        out["success"] = np.array([bool(s) if k == COMPONENT_COMPLETED else True for s, k in zip(rec["reserved"], kind)], dtype=bool) if n else np.zeros(0, dtype=bool)
    return out


def _component_rows(kind: int):
    """the scanned parameters of a component kind (0 steam generator, 2 condenser), in row order"""
    from ._lib import CMAINT_PARAMS, COMPONENT_KINDS
    return [name for k, name in CMAINT_PARAMS if k == COMPONENT_KINDS[kind]]


def summary_keys(keys, operator: bool = False):
    """the keys of a summary as (catalog, action, unit, kinds) integers (include/npb_maint.h npb_maint_summary_key_t): each a plain
    feedwater action name, a (catalog_name, action_or_None, unit_or_None) triple (``_lib.summary_key``), or four integers taken as they are"""
    from ._lib import summary_key
    return [tuple(int(x) for x in k) if not isinstance(k, str) and len(k) == 4 else summary_key(k, operator=operator) for k in keys]


def summarize(records: np.ndarray, keys, n_plants: int, since_minutes: float = 0.0, operator: bool = False) -> Dict[str, np.ndarray]:
    """The per-plant work-order summary of drained records: what the device folds the log into (npb_set_maintenance_summary), restated
    over numpy -- the reduction the device's tables are held to, bit for bit.  Per key j and plant p: ``first_created`` /
    ``first_completed`` (float64 [n_keys, n_plants], +inf = never) and ``n_created`` / ``n_completed`` (int32).  A record's catalog follows
    from its kind (0, 1, 2 feedwater; 3, 5, 6 component; 4 turbine); it matches a key of its catalog whose ``kinds`` mask has its kind and
    whose action and unit are its own or -1; a creation kind (CREATED, COMPONENT_CREATED) feeds the created pair, any other the completed
    pair; records with ``time < since_minutes`` are dropped (the data-gen runner's tracking_start_hours,
    maintenance_scenario_runner.py:431-468).  ``keys`` as ``summary_keys`` takes them."""
    from ._lib import SUMMARY_CATALOGS, SUMMARY_CREATION_KINDS, SUMMARY_KINDS
    rec = np.asarray(records, dtype=EVENT_DTYPE)
    K = summary_keys(keys, operator=operator)
    n = int(n_plants)
    out = {"first_created": np.full((len(K), n), np.inf), "first_completed": np.full((len(K), n), np.inf),
           "n_created": np.zeros((len(K), n), dtype=np.int32), "n_completed": np.zeros((len(K), n), dtype=np.int32)}
    catalog_of = np.full(256, -1, dtype=np.int64)
    for c, name in enumerate(SUMMARY_CATALOGS):
        for k in SUMMARY_KINDS[name][0] + SUMMARY_KINDS[name][1]:
            catalog_of[k] = c
    kind = rec["kind"].astype(np.int64)
    live = (~(rec["time"] < since_minutes)) & (rec["plant"] >= 0) & (rec["plant"] < n) & (catalog_of[kind] >= 0)
    creation = np.isin(kind, SUMMARY_CREATION_KINDS)
    for j, (catalog, action, unit, kinds) in enumerate(K):
        m = live & (catalog_of[kind] == catalog) & (((kinds >> np.minimum(kind, 62)) & 1) == 1)
        if action >= 0:
            m &= rec["action"] == action
        if unit >= 0:
            m &= rec["pump"] == unit
        for sel, first, count in ((m & creation, "first_created", "n_created"), (m & ~creation, "first_completed", "n_completed")):
            np.minimum.at(out[first][j], rec["plant"][sel], rec["time"][sel])
            np.add.at(out[count][j], rec["plant"][sel], 1)
    return out


def table(cols: Dict[str, np.ndarray]):
    """pyarrow Table of ``columns``' output"""
    import pyarrow as pa
    return pa.table({k: pa.array(list(v) if v.dtype == object else v) for k, v in cols.items()})


def write(cols: Dict[str, np.ndarray], path: str) -> None:
    """CSV (``.csv``) or Parquet (anything else), as StateLog.write_parquet writes its table"""
    t = table(cols)
    if path.endswith(".csv"):
        import pyarrow.csv as pcsv
        pcsv.write_csv(t, path)
    else:
        import pyarrow.parquet as pq
        pq.write_table(t, path)
