"""CPU: the numpy statement of the controls (nuclear_sim_amd.controls), the request function (_lib.controls_request), the two column words,
and the statement against the C oracle: moving an actuator in front of a step with NO_ACTION is the step with that action, bit for bit."""
import numpy as np
import pytest

from nuclear_sim_amd import _lib, controls


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _spec(axes, interval=1, dtype="float64"):
    return {"interval": interval, "dtype": dtype, "axes": axes}


def _one(axis, x, pos, target=None, **kw):
    """one step of a one-axis Decoder over the inputs x against the positions pos"""
    x, pos = np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(pos, dtype=np.float64))
    dec = controls.Decoder(_spec([axis]), len(x), **kw)
    out = dec.step(x.reshape(-1, 1), {axis["target"]: pos} if axis["kind"] != "column" else {})
    return out


def test_the_transform_order_nan_clip_and_deadband():
    D = controls.axis("rate", "rod", scale=2.0, offset=0.25, lo=-0.5, hi=0.75, nan_to=0.125, deadband=0.25)
    x = np.array([np.nan, 0.1, -1.0, 1.0, 0.0, -0.25, -0.2, 1e-17])
    y, rep = controls.transform(D, x)
    # NaN -> nan_to BEFORE the affine map: 0.125 * 2 + 0.25; both clip ends; fabs(y) == deadband stays, below it is zeroed
    want = np.array([0.5, 0.1 * 2.0 + 0.25, -0.5, 0.75, 0.25, -0.25, 0.0, 0.25])
    assert np.array_equal(_bits(y), _bits(want))
    assert rep[0] & controls.NAN_IN and not rep[1] & controls.NAN_IN
    assert rep[2] & controls.CLIP_LO and rep[3] & controls.CLIP_HI and not rep[1] & (controls.CLIP_LO | controls.CLIP_HI)
    assert rep[6] & controls.DEADBAND and not rep[4] & controls.DEADBAND and not rep[5] & controls.DEADBAND
    # the product is rounded before the sum: x * scale + offset in two steps
    D2 = controls.axis("column", "power_setpoint", scale=1.0 / 3.0, offset=1e16)
    x2 = np.array([3.0000000000000004])
    assert controls.transform(D2, x2)[0][0] == (x2[0] * (1.0 / 3.0)) + 1e16
    # a target or a column has no deadband and no default clip
    y3, _ = controls.transform(controls.axis("target", "valve", deadband=0.0), np.array([1e9, -1e9]))
    assert y3.tolist() == [1e9, -1e9]
    # float32 input is widened first
    xf = np.array([0.1], dtype=np.float32)
    assert controls.transform(controls.axis("column", "cooling_water_temp", scale=3.0), xf)[0][0] == np.float64(xf[0]) * 3.0


@pytest.mark.parametrize("actuator", controls.ACTUATORS)
def test_rate_in_both_directions_and_into_each_range_limit(actuator):
    lo, hi = controls.RANGES[actuator]
    speed, dt = controls.DEFAULT_SPEEDS[actuator], 2.0
    mid = 0.5 * (lo + hi)
    D = controls.axis("rate", actuator)
    out = _one(D, [0.3, -0.7, 0.0, 1.0, -1.0], [mid, mid, mid, hi - 0.5 * speed, lo + 0.5 * speed], dt=dt)
    want = [mid + speed * dt * 0.3, mid - speed * dt * 0.7, mid, hi, lo]
    assert np.array_equal(_bits(out["members"][actuator]), _bits(want))
    rep = out["report"][0]
    assert rep[0] & controls.RATE_UP and rep[1] & controls.RATE_DOWN and rep[2] & controls.RATE_ZERO
    assert rep[3] & controls.LIMIT_HI and rep[4] & controls.LIMIT_LO and not rep[0] & controls.LIMIT_HI and not rep[1] & controls.LIMIT_LO
    assert np.array_equal(out["held"][0], [0.3, -0.7, 0.0, 1.0, -1.0])


@pytest.mark.parametrize("actuator", controls.ACTUATORS)
def test_target_above_below_equal_within_and_beyond_one_move_and_out_of_range(actuator):
    lo, hi = controls.RANGES[actuator]
    speed, dt, mag = controls.DEFAULT_SPEEDS[actuator], 1.0, 0.5
    one = speed * dt * mag
    mid = 0.5 * (lo + hi)
    D = controls.axis("target", actuator, max_magnitude=mag)
    y = [mid + 0.3 * one, mid - 0.3 * one, mid, mid + 7 * one, mid - 7 * one, hi + 10.0, lo - 10.0]
    pos = [mid, mid, mid, mid, mid, hi - 0.25 * one, lo + 0.25 * one]
    out = _one(D, y, pos, dt=dt)
    want = [y[0], y[1], mid, mid + one, mid - one, hi, lo]
    assert np.array_equal(_bits(out["members"][actuator]), _bits(want))
    rep = out["report"][0]
    assert rep[0] & controls.TARGET_REACHED and rep[1] & controls.TARGET_REACHED and rep[2] & controls.TARGET_EQUAL
    assert rep[3] & controls.TARGET_NOT_REACHED and rep[4] & controls.TARGET_NOT_REACHED
    assert rep[5] & controls.TARGET_OUT_OF_RANGE and rep[6] & controls.TARGET_OUT_OF_RANGE


def test_float32_storage_rounds_a_moved_member_and_keeps_an_unmoved_one():
    pos = np.array([np.float64(np.float32(50.1)), np.float64(np.float32(50.1))])
    out = _one(controls.axis("rate", "rod"), [0.137, 0.0], pos, storage="float32")
    moved = pos[0] + 5.0 * 1.0 * 0.137
    assert out["members"]["rod"][0] == np.float64(np.float32(moved)) != moved
    assert _bits(out["members"]["rod"])[1] == _bits(pos)[1]


def test_columns():
    axes = [controls.axis("column", "power_setpoint", scale=10.0, offset=90.0, lo=80.0, hi=100.0), controls.axis("column", "cooling_water_temp", offset=25.0)]
    dec = controls.Decoder(_spec(axes), 3)
    out = dec.step(np.array([[0.5, 1.0], [5.0, -1.0], [np.nan, 0.0]]), {})
    assert out["columns"]["power_setpoint"].tolist() == [95.0, 100.0, 90.0] and out["columns"]["cooling_water_temp"].tolist() == [26.0, 24.0, 25.0]
    assert out["members"] == {} and (out["report"] & controls.COLUMN).all()


def test_a_value_axis_is_only_held():
    spec = _lib.controls_request([(None, "value", {"scale": 2.0}), ("rod", "rate"), (None, "value")])
    dec = controls.Decoder(spec, 2)
    out = dec.step(np.array([[0.5, 0.0, 7.0], [np.nan, 0.0, -3.0]]), {"rod": np.array([50.0, 50.0])})
    assert out["held"].tolist() == [[1.0, 0.0], [0.0, 0.0], [7.0, -3.0]] and out["columns"] == {} and list(out["members"]) == ["rod"]
    assert (out["report"][[0, 2]] & controls.VALUE).all() and not (out["report"][1] & controls.VALUE).any()


@pytest.mark.parametrize("K", [1, 3])
def test_the_hold_across_an_unprimed_step(K):
    n = 4
    dec = controls.Decoder(_spec([controls.axis("rate", "valve"), controls.axis("target", "rod", max_magnitude=1.0)], interval=K), n)
    rng = np.random.default_rng(K)
    valve, rod = np.full(n, 50.0), np.full(n, 50.0)
    index = np.zeros(n, dtype=np.int32)
    age = np.zeros(n, dtype=np.int64)
    held = prev = None
    for t in range(8):
        x = np.stack([rng.uniform(-1, 1, n), rng.uniform(30, 70, n)], axis=1)
        if t == 4:
            dec.clear(np.array([0, 1, 0, 0]))      # plant 1 cleared
            age[1] = 0
        if t == 5:
            index[2] += 1                           # plant 2 starts a new episode
            age[2] = 0
        unprimed = (age == 0) & ((t == 0) | ((t == 4) & (np.arange(n) == 1)) | ((t == 5) & (np.arange(n) == 2)))
        latch = age % K == 0
        out = dec.step(x, {"valve": valve, "rod": rod}, index)
        want_held = np.where(latch, x.T, held if held is not None else x.T)
        want_prev = np.where(latch, np.where(unprimed, x.T, held if held is not None else x.T), prev if prev is not None else x.T)
        assert np.array_equal(_bits(out["held"]), _bits(want_held)), t
        assert np.array_equal(_bits(out["prev"]), _bits(want_prev)), t
        assert np.array_equal((out["report"][0] & controls.LATCHED) != 0, latch) and np.array_equal((out["report"][0] & controls.HELD) != 0, ~latch)
        assert np.array_equal((out["report"][0] & controls.UNPRIMED) != 0, unprimed), t
        # a held rate repeats its move, a held target keeps moving towards its target
        assert np.array_equal(_bits(out["members"]["valve"]), _bits(np.where(want_held[0] > 0, np.minimum(100.0, valve + 10.0 * want_held[0]),
                                                                              np.maximum(0.0, valve - 10.0 * -want_held[0])))), t
        assert np.all(np.abs(out["members"]["rod"] - want_held[1]) <= np.abs(rod - want_held[1]))
        held, prev = want_held.copy(), want_prev.copy()
        valve, rod = out["members"]["valve"], out["members"]["rod"]
        age += 1
        assert np.array_equal(dec.age, age) and dec.primed.all() and np.array_equal(dec.seen, index)
    if K == 3:
        assert not np.array_equal(dec.age, np.full(n, 8))      # the cleared and the restarted plant run on a phase of their own


REFUSALS = [
    (dict(axes=[]), "controls take 1 to 8 axes, not 0"),
    (dict(axes=[("rod", "rate")] * 9), "controls take 1 to 8 axes, not 9"),
    (dict(axes=[("rod", "rate")], interval=0), "the interval must be 1 .. 64, not 0"),
    (dict(axes=[("rod", "rate")], interval=65), "the interval must be 1 .. 64, not 65"),
    (dict(axes=[("rod", "rate")], interval=True), "the interval must be 1 .. 64, not True"),
    (dict(axes=[("rod", "rate")], dtype="float16"), "the input type must be float32 or float64"),
    (dict(axes=["rod"]), "an axis is \\(target, kind\\) or \\(target, kind, options\\)"),
    (dict(axes=[("rod", "rate", 3)]), "an axis is \\(target, kind\\) or \\(target, kind, options\\)"),
    (dict(axes=[("rod", "speed")]), "unknown kind 'speed'"),
    (dict(axes=[("pump", "rate")]), "unknown actuator 'pump'"),
    (dict(axes=[("rod", "column")]), "unknown input 'rod'"),
    (dict(axes=[("rod", "value")]), "unknown actuator 'rod'"),
    (dict(axes=[("power_setpoint", "target")]), "unknown actuator 'power_setpoint'"),
    (dict(axes=[("rod", "rate"), ("rod", "target")]), "'rod' is already taken by axis 0"),
    (dict(axes=[("power_setpoint", "column"), ("power_setpoint", "column")]), "'power_setpoint' is already taken by axis 0"),
    (dict(axes=[("rod", "rate", {"gain": 1.0})]), "unknown option 'gain'"),
    (dict(axes=[("rod", "rate", {"scale": np.nan})]), "the scale must be finite"),
    (dict(axes=[("rod", "rate", {"scale": "1"})]), "the scale must be a number"),
    (dict(axes=[("rod", "rate", {"offset": np.inf})]), "the offset must be finite"),
    (dict(axes=[("rod", "rate", {"nan_to": np.nan})]), "nan_to must be finite"),
    (dict(axes=[("rod", "rate", {"deadband": np.inf})]), "the deadband must be finite"),
    (dict(axes=[("rod", "rate", {"deadband": -0.1})]), "a negative deadband"),
    (dict(axes=[("rod", "target", {"deadband": 0.1})]), "'deadband' is a rate's option"),
    (dict(axes=[("rod", "target", {"max_magnitude": -1.0})]), "a negative max_magnitude"),
    (dict(axes=[("rod", "target", {"max_magnitude": np.nan})]), "max_magnitude must be finite"),
    (dict(axes=[("rod", "rate", {"max_magnitude": 1.0})]), "'max_magnitude' is a target's option"),
    (dict(axes=[("rod", "rate", {"clip": 1.0})]), "'clip' is \\(lo, hi\\)"),
    (dict(axes=[("rod", "rate", {"clip": (np.nan, 1.0)})]), "the clip limits must be numbers"),
    (dict(axes=[("rod", "rate", {"clip": (1.0, -1.0)})]), "a clip with lo > hi"),
    (dict(axes=[("power_setpoint", "column")], heat_source=_lib.HEAT_EXTERNAL), "the power_setpoint column carries the plugin's power"),
]


@pytest.mark.parametrize("kwargs, message", REFUSALS)
def test_every_refusal_of_the_request(kwargs, message):
    with pytest.raises(ValueError, match=message):
        _lib.controls_request(**kwargs)


def test_the_request_fills_the_defaults_and_feeds_the_decoder():
    req = _lib.controls_request([("rod", "rate"), ("valve", "target", {"max_magnitude": 0.5, "clip": (0, None)}),
                                 ("power_setpoint", "column", {"scale": 10.0, "offset": 90.0, "clip": (80.0, 100.0)}),
                                 ("cooling_water_temp", "column")], interval=4, dtype=np.float64)
    assert req["interval"] == 4 and req["dtype"] == "float64"
    assert req["axes"][0] == controls.axis("rate", "rod") and (req["axes"][0]["lo"], req["axes"][0]["hi"]) == (-1.0, 1.0)
    assert req["axes"][1] == controls.axis("target", "valve", max_magnitude=0.5, lo=0.0)
    assert req["axes"][3] == controls.axis("column", "cooling_water_temp")
    controls.check(req)
    assert _lib.controls_request([("power_setpoint", "column")], heat_source=_lib.HEAT_EXTERNAL - 1)["dtype"] == "float32"
    import torch
    assert _lib.controls_request([("boron", "rate")], dtype=torch.float64)["dtype"] == "float64"
    for name, table in (("KINDS", _lib.CONTROL_KINDS), ("ACTUATORS", _lib.CONTROL_ACTUATORS), ("INPUTS", _lib.CONTROL_INPUTS), ("DTYPES", _lib.CONTROL_DTYPES)):
        assert [table[k] for k in getattr(controls, name)] == list(range(len(table))), name


def test_the_control_words_need_controls():
    for word in (("control", 0), ("control_prev", 1)):
        with pytest.raises(ValueError) as today:
            _lib.column_word(("nonsense", 0))
        with pytest.raises(ValueError) as e:
            _lib.column_word(word)
        assert str(e.value) == str(today.value).replace("('nonsense', 0)", repr(word))      # today's exact text
        assert _lib.column_word(word, controls=2) == {"member": None, "side": (word[0], word[1], 1, "f64"), "integer": False}
    with pytest.raises(ValueError, match="the controls' axes are 0 .. 1, not 2"):
        _lib.column_word(("control", 2), controls=2)
    with pytest.raises(ValueError, match="unknown column"):
        _lib.task_request(reward=[(("control", 0), 1.0)])
    # the four request functions take the axis count
    assert _lib.task_request(reward=[(("control", 0), -0.1, "abs_err", 0.0), (("control", 0), -1.0, "sq_err", ("control_prev", 0))], controls=1)["columns"][0]["side"][0] == "control"
    assert _lib.features_request([("control", 1), ("control_prev", 0)], controls=2)["columns"][1]["side"] == ("control_prev", 0, 1, "f64")
    assert _lib.column_stats_request([("control", 0)], controls=1)["sides"] == [("control", 0, 1)]
    assert _lib.event_windows_request([("control_prev", 0)], [("done",)], 1, 1, controls=1)["sides"] == [("control_prev", 0, 1)]
    # in a feature's fresh frame the two words take `fresh`, as every side column that is not live
    assert _lib.features_request([("control", 0)], controls=1)["spec"]["columns"][0]["live"] is False


@pytest.mark.parametrize("code", [0, 1, 2, 3, 4, 5, 9, 10])
def test_the_statement_then_a_step_with_no_action_is_the_oracles_step_with_the_action(code):
    """For each RATE action code: "Decoder's new member, then the oracle's step with NO_ACTION" equals "the oracle's step with (code,
    magnitude)" bit for bit on every state member -- the four members are read only behind the step's own actuator move"""
    from oracle import npo
    actuator = [a for a in controls.ACTUATORS if code in (controls.UP_CODES[a], controls.DOWN_CODES[a])][0]
    up = code == controls.UP_CODES[actuator]
    n = 6
    rng = np.random.default_rng(code)
    P = npo.Params()
    P.dt = 2.0
    a, b = npo.OraclePlants(n, P), npo.OraclePlants(n, P)
    lo, hi = controls.RANGES[actuator]
    start = rng.uniform(lo, hi, n)
    start[0], start[1] = (hi, hi - 1e-3) if up else (lo, lo + 1e-3)      # at and into the range limit
    for o in (a, b):
        o.set(controls.MEMBERS[actuator], start)
    dec = controls.Decoder(_spec([controls.axis("rate", actuator)]), n, dt=2.0,
                           speeds={"rod": P.max_control_rod_speed, "flow": P.max_flow_change_rate, "valve": P.max_valve_speed})
    NO_ACTION = 8
    for t in range(4):
        mag = rng.uniform(0.0, 1.0, n)
        mag[2] = 0.0
        sp = rng.uniform(85, 100, n)
        pos = np.array([a.get(controls.MEMBERS[actuator], plant=p) for p in range(n)])
        assert np.array_equal(_bits(pos), _bits([b.get(controls.MEMBERS[actuator], plant=p) for p in range(n)]))
        out = dec.step((mag if up else -mag).reshape(n, 1), {actuator: pos})
        a.set(controls.MEMBERS[actuator], out["members"][actuator])
        ra = a.step(action=NO_ACTION, magnitude=0.0, setpoint=sp)
        rb = b.step(action=code, magnitude=mag, setpoint=sp)
        for x, y in zip(ra, rb):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (t, code)
        (fa, ia), (fb, ib) = a.state_all(), b.state_all()
        assert np.array_equal(_bits(fa), _bits(fb)) and np.array_equal(ia, ib), (t, code)
    assert out["report"][0, 0] & (controls.LIMIT_HI if up else controls.LIMIT_LO) and out["report"][0, 2] & controls.RATE_ZERO
