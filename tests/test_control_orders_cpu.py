"""CPU: the numpy statement of the order rules on the controls' axes (nuclear_sim_amd.controls.Orders / orders_check), the caller's words
(_lib.control_orders_request) and the column word ("order", r).  No library, no device.

The recurrence is checked on hand-made held / latch / restart arrays against values worked out by hand: fire = latch and y > threshold
and (c == NEVER or c >= min_interval), c = NEVER on a restart, since = 1 on a firing, else c + 1 (NEVER stays)."""
import numpy as np
import pytest

from nuclear_sim_amd import _lib, controls

NEVER = controls.NEVER
SPEC = {"interval": 1, "dtype": "float32", "axes": [controls.axis("rate", "rod"), controls.axis("value", None), controls.axis("value", None),
                                                    controls.axis("column", "cooling_water_temp")]}


def _rules(*orders):
    return _lib.control_orders_request(orders)


def _run(rules, held_steps, latch_steps=None, restart_steps=None, n=None):
    """fire [T, R, n] and since [T, R, n] of an Orders over the steps; held_steps [T, A, n]"""
    held_steps = np.asarray(held_steps, dtype=np.float64)
    T, _A, n = held_steps.shape
    O = controls.Orders(rules, SPEC, n)
    fires, sinces = [], []
    for t in range(T):
        latch = np.ones(n, bool) if latch_steps is None else np.asarray(latch_steps[t], bool)
        restart = (np.full(n, t == 0)) if restart_steps is None else np.asarray(restart_steps[t], bool)
        fires.append(O.step(held_steps[t], latch, restart))
        sinces.append(O.since.copy())
    return np.array(fires), np.array(sinces)


def _held(axis1, axis2=None):
    """[T, 4, n] with the two VALUE axes filled from [T, n] arrays"""
    a1 = np.asarray(axis1, dtype=np.float64)
    out = np.zeros((a1.shape[0], 4, a1.shape[1]))
    out[:, 1] = a1
    out[:, 2] = a1 if axis2 is None else np.asarray(axis2, dtype=np.float64)
    return out


def test_the_comparison_is_strict_and_a_nan_never_fires():
    rules = _rules((1, "pump", "oil_top_off", {"threshold": 0.5}))
    y = [[0.5, np.nextafter(0.5, 1.0), np.nextafter(0.5, 0.0), np.nan, np.inf, -np.inf, 0.0]]
    fire, since = _run(rules, _held(y))
    assert fire[0, 0].tolist() == [False, True, False, False, True, False, False]
    assert since[0, 0].tolist() == [NEVER, 1, NEVER, NEVER, 1, NEVER, NEVER]
    assert fire.dtype == bool and since.dtype == np.int32


def test_never_fires_at_once_whatever_the_interval_and_since_counts_from_the_firing():
    rules = _rules((1, "pump", "oil_change", {"min_interval": 1}), (1, "pump", "oil_change", {"min_interval": 2}),
                   (1, "pump", "oil_change", {"min_interval": 5}))
    T = 12
    fire, since = _run(rules, _held(np.ones((T, 1))))      # always above: each rule fires every min_interval steps from step 0
    for r, K in enumerate((1, 2, 5)):
        assert fire[:, r, 0].tolist() == [t % K == 0 for t in range(T)], K
        assert since[:, r, 0].tolist() == [t % K + 1 for t in range(T)], K


def test_min_interval_1_2_and_5_across_a_restart():
    rules = _rules((1, "pump", "oil_change", {"min_interval": 1}), (1, "pump", "oil_change", {"min_interval": 2}),
                   (1, "pump", "oil_change", {"min_interval": 5}))
    T = 10
    restart = np.zeros((T, 2), bool)
    restart[0] = True
    restart[3, 1] = True      # plant 1 restarts on step 3; plant 0 never again
    fire, since = _run(rules, _held(np.ones((T, 2))), restart_steps=restart)
    assert fire[:, 1, 0].tolist() == [t % 2 == 0 for t in range(T)]
    assert fire[:, 2, 0].tolist() == [t % 5 == 0 for t in range(T)]
    # plant 1: the restart makes every rule fire on step 3 again, and the intervals count from there
    assert fire[:, 0, 1].all()
    assert fire[:, 1, 1].tolist() == [True, False, True, True, False, True, False, True, False, True]
    assert fire[:, 2, 1].tolist() == [True, False, False, True, False, False, False, False, True, False]
    assert since[:, 2, 1].tolist() == [1, 2, 3, 1, 2, 3, 4, 5, 1, 2]


def test_a_restart_without_a_firing_leaves_never_and_never_stays():
    rules = _rules((1, "pump", "oil_change", {"min_interval": 3}))
    y = np.array([[1.0], [0.0], [0.0], [0.0], [1.0], [0.0]])
    restart = np.array([[True], [False], [True], [False], [False], [False]])
    fire, since = _run(rules, _held(y), restart_steps=restart)
    assert fire[:, 0, 0].tolist() == [True, False, False, False, True, False]
    assert since[:, 0, 0].tolist() == [1, 2, NEVER, NEVER, 1, 2]      # step 2 forgets the count; NEVER + 1 is NEVER; step 4 fires at once


def test_since_saturates_below_never():
    rules = _rules((1, "pump", "oil_change"))
    O = controls.Orders(rules, SPEC, 3)
    O.load_state({"since": np.array([[NEVER - 2, NEVER - 1, NEVER]], dtype=np.int32)})
    fire = O.step(np.zeros((4, 3)), np.ones(3, bool), np.zeros(3, bool))
    assert not fire.any() and O.since.tolist() == [[NEVER - 1, NEVER - 1, NEVER]]
    assert O.state()["since"].dtype == np.int32


def test_a_held_step_never_fires_and_still_counts():
    rules = _rules((1, "pump", "oil_change", {"min_interval": 2}))
    T = 8
    latch = np.array([[t % 3 == 0] for t in range(T)])      # the hold of an interval of 3
    fire, since = _run(rules, _held(np.ones((T, 1))), latch_steps=latch)
    assert fire[:, 0, 0].tolist() == [True, False, False, True, False, False, True, False]
    assert since[:, 0, 0].tolist() == [1, 2, 3, 1, 2, 3, 1, 2]
    # with the Decoder: latch and restart are its own
    spec = dict(SPEC, interval=3)
    D, O = controls.Decoder(spec, 2), controls.Orders(rules, spec, 2)
    x = np.zeros((2, 4)); x[:, 1] = 1.0
    got = []
    for t in range(7):
        if t == 4:
            D.clear([0, 1])      # plant 1's hold restarts: it latches, and fires, out of turn
        out = D.step(x, {"rod": np.full(2, 50.0)})
        assert set(out) >= {"members", "columns", "held", "prev", "report", "latch", "restart"}
        got.append(O.step(out["held"], out["latch"], out["restart"])[0].tolist())
    assert got == [[True, True], [False, False], [False, False], [True, True], [False, True], [False, False], [True, False]]


def test_two_rules_on_one_axis_have_their_own_thresholds_and_counts():
    rules = _rules((2, "pump", "oil_top_off", {"threshold": 0.25, "min_interval": 3}), (2, "steam_generator", "tsp_chemical_cleaning", {"threshold": 0.75}))
    y = np.array([[0.5, 1.0], [0.5, 1.0], [1.0, 0.0], [1.0, 1.0]])
    fire, since = _run(rules, _held(np.zeros_like(y), y))
    assert fire[:, 0].tolist() == [[True, True], [False, False], [False, False], [True, True]]
    assert fire[:, 1].tolist() == [[False, True], [False, True], [True, False], [True, True]]
    assert since[3].tolist() == [[1, 1], [1, 1]] and since[1, 1].tolist() == [NEVER, 1]


def test_calls_lists_the_perform_calls_in_rule_order():
    rules = _rules((1, "pump", "bearing_replacement", {"unit": 2, "bearing": "thrust_bearing"}),
                   (1, "pump", "oil_top_off", {"unit": 2, "target_level": 90.0}),
                   (2, "condenser", "condenser_tube_cleaning", {"cleaning_type": "mechanical"}),
                   (2, "ejector", "vacuum_ejector_cleaning", {"unit": 1}),
                   (1, "bearing", "thrust_bearing_adjustment", {"unit": 2}),
                   (2, "stage", "overhaul", {"unit": 13}))
    O = controls.Orders(rules, SPEC, 3)
    fire = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 0, 0], [1, 1, 1]], dtype=bool)
    calls = O.calls(fire)
    assert [name for name, _kw in calls] == ["perform_maintenance", "perform_maintenance", "perform_component_maintenance",
                                             "perform_component_maintenance", "perform_turbine_maintenance", "perform_turbine_maintenance"]
    for r, (_name, kw) in enumerate(calls):
        assert kw["mask"].tolist() == fire[r].astype(int).tolist() and kw["mask"].dtype == np.uint8
    assert {k: v for k, v in calls[0][1].items() if k != "mask"} == {"action": _lib.MAINT_ACTION_NAMES.index("bearing_replacement"), "pump": 2,
                                                                     "bearing": 3, "target_level": 95.0}
    assert calls[1][1]["target_level"] == 90.0 and calls[1][1]["bearing"] == 0
    assert calls[2][1]["component"] == "condenser" and calls[2][1]["cleaning_type"] == _lib.CLEANING_TYPES["mechanical"]
    assert calls[2][1]["action"] == _lib.COMPONENT_ACTIONS.index(("condenser", "condenser_tube_cleaning"))
    assert (calls[3][1]["component"], calls[3][1]["unit"]) == ("ejector", 1)
    assert (calls[4][1]["component"], calls[4][1]["unit"]) == ("bearing", 2)
    assert (calls[5][1]["component"], calls[5][1]["unit"], calls[5][1]["action"]) == ("stage", 13, _lib.TURBINE_ACTIONS.index(("stage", "overhaul")))


def test_the_request_resolves_names_indices_and_defaults_and_keeps_the_not_offered_refusals():
    R = _rules((1, "pump", "oil_top_off"))[0]
    assert R == {"axis": 1, "family": "pump", "action": 1, "unit": 0, "option": 0, "amount": 95.0, "threshold": 0.0, "min_interval": 1}
    assert _rules((2, "lubrication", 13, {"threshold": -0.5}))[0]["action"] == 13
    with pytest.raises(ValueError, match="is not offered on the device"):
        _rules((1, "steam_generator", "eddy_current_testing"))
    with pytest.raises(ValueError, match="is not offered on the device"):
        _rules((1, "stage", "cleaning"))
    with pytest.raises(ValueError, match="unknown maintenance action"):
        _rules((1, "pump", "polish"))
    with pytest.raises(ValueError, match="unknown component"):
        _rules((1, "reactor", "oil_change"))
    with pytest.raises(ValueError, match="unknown option"):
        _rules((1, "pump", "oil_change", {"level": 3}))
    with pytest.raises(ValueError, match="unknown bearing"):
        _rules((1, "pump", "bearing_replacement", {"bearing": "left"}))
    with pytest.raises(ValueError, match="is a bearing action, not a stage one"):
        _rules((1, "stage", _lib.TURBINE_ACTIONS.index(("bearing", "bearing_alignment"))))
    with pytest.raises(ValueError, match="1 to 8"):
        _rules()
    with pytest.raises(ValueError, match="1 to 8"):
        _rules(*[(1, "pump", "oil_change")] * 9)


def _bad(change, **kw):
    rules = _rules((1, "pump", "bearing_replacement", {"unit": 3, "bearing": 3}), (2, "steam_generator", "scale_removal", {"unit": 2}),
                   (2, "condenser", "condenser_tube_cleaning"), (1, "bearing", "thrust_bearing_adjustment", {"unit": 2}), (2, "stage", "overhaul", {"unit": 13}))
    controls.orders_check(rules, SPEC, 70, kw.get("mode", "full"))      # valid as it stands (in the full mode)
    change(rules)
    return rules


REFUSALS = [
    ("an axis that is none", lambda R: R[0].update(axis=4), "the controls' axes are 0 .. 3"),
    ("a RATE axis", lambda R: R[0].update(axis=0), "a rule reads a 'value' axis"),
    ("a COLUMN axis", lambda R: R[1].update(axis=3), "a rule reads a 'value' axis"),
    ("an unknown family", lambda R: R[0].update(family="valve"), "unknown family"),
    ("a pump action outside the catalog", lambda R: R[0].update(action=18), "outside the catalog"),
    ("a pump action without a handler", lambda R: R[0].update(action=_lib.MAINT_ACTION_NAMES.index("routine_maintenance")), "has no handler"),
    ("pump 4", lambda R: R[0].update(unit=4), "does not exist"),
    ("bearing 4", lambda R: R[0].update(option=4), "outside its range"),
    ("a component action outside the catalog", lambda R: R[1].update(action=len(_lib.COMPONENT_ACTIONS)), "outside the catalog"),
    ("generator 3", lambda R: R[1].update(unit=3), "does not exist"),
    ("a turbine action outside the catalog", lambda R: R[4].update(action=-1), "outside the catalog"),
    ("stage 14", lambda R: R[4].update(unit=14), "does not exist"),
    ("a thrust adjustment on a journal bearing", lambda R: R[3].update(unit=0), "a thrust adjustment on journal bearing"),
    ("a NaN threshold", lambda R: R[2].update(threshold=float("nan")), "must be finite"),
    ("an infinite threshold", lambda R: R[2].update(threshold=float("inf")), "must be finite"),
    ("min_interval 0", lambda R: R[2].update(min_interval=0), "min_interval must be an int >= 1"),
    ("a float min_interval", lambda R: R[2].update(min_interval=2.0), "min_interval must be an int >= 1"),
    ("no rules", lambda R: R.clear(), "1 to 8"),
    ("nine rules", lambda R: R.extend([R[0]] * 4), "1 to 8"),
]


@pytest.mark.parametrize("name,change,reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_orders_check_gives_every_refusal(name, change, reason):
    rules = _bad(change)
    with pytest.raises(ValueError, match=reason):
        controls.orders_check(rules, SPEC, 70, "full")
    with pytest.raises(ValueError, match=reason):
        controls.Orders(rules, SPEC, 70)


def test_orders_check_refuses_what_the_mode_does_not_step_and_a_handle_without_controls():
    rules = _bad(lambda R: None)
    with pytest.raises(ValueError, match="does not step the condenser"):
        controls.orders_check(rules, SPEC, 70, "primary_sg")
    with pytest.raises(ValueError, match="does not step the turbine"):
        controls.orders_check(rules[:2] + rules[3:], SPEC, 70, "primary_sg")
    controls.orders_check(rules[:2], SPEC, 70, "primary_sg")      # a pump and a generator
    with pytest.raises(ValueError, match="does not step the steam_generator"):
        controls.orders_check(rules[:2], SPEC, 70, "primary")
    controls.orders_check(rules[:1], SPEC, 70, "primary")         # an operator's pump call succeeds in every mode
    with pytest.raises(ValueError, match="need controls"):
        controls.orders_check(rules, None, 70)
    with pytest.raises(ValueError, match="n_plants"):
        controls.orders_check(rules, SPEC, 0)


def test_order_is_a_column_word_while_rules_are_set_and_its_range_check_refuses():
    assert _lib.column_word(("order", 0), orders=1) == {"member": None, "side": ("order", 0, 1, "f64"), "integer": False}
    assert _lib.column_word(("order", 7), orders=8)["side"] == ("order", 7, 1, "f64")
    for bad in (2, -1, True, 1.0, "0"):
        with pytest.raises(ValueError, match="the order rules are 0 .. 1"):
            _lib.column_word(("order", bad), orders=2)
    with pytest.raises(ValueError, match="unknown column"):      # no word without rules
        _lib.column_word(("order", 0))
    # every vocabulary takes it
    assert _lib.task_request(reward=[(("order", 1), -0.01)], orders=2)["columns"][0]["side"][0] == "order"
    assert _lib.features_request([("order", 0)], orders=1)["columns"][0]["side"][0] == "order"
    assert _lib.column_stats_request([("order", 0)], orders=1)["sides"] == [("order", 0, 1)]
    with pytest.raises(ValueError, match="unknown column"):
        _lib.features_request([("order", 0)])
