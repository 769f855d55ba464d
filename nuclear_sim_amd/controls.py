"""Caller-defined policy outputs, stated once in numpy: what the device does in front of every step while ``env.set_controls`` is on
(npb_set_controls, nuclear_sim_amd/csrc/npd_controls.h).  Host only.

A ``spec`` is ``{"interval": K, "dtype": "float32" | "float64", "axes": [...]}``; axis a reads ``x[p, a]`` of the policy's output, widened
to float64, and is ``{"kind": k, "target": t, "scale", "offset", "lo", "hi", "nan_to", "deadband", "max_magnitude"}``.  The transform, every
step rounded on its own: a NaN x becomes ``nan_to``; ``y = x * scale + offset``; ``y = lo if y < lo else y``, then ``y = hi if y > hi else
y``; for "rate" only, ``abs(y) < deadband`` gives 0.0.  Then by kind:

  "rate"      target an actuator of ``ACTUATORS``: y > 0 is the reference's move with the actuator's increasing ControlAction code at
              magnitude y, y < 0 the decreasing code at -y, y == 0 nothing
  "target"    y is a position: the move at ``max_magnitude`` towards y, stopped at y -- ``min(up, y)`` above the position, ``max(down, y)``
              below it, nothing where they are equal; the actuator's range limit comes with up and down
  "column"    target an input of ``INPUTS``: y is that plant's value of the step's input column
  "value"     target None: y moves nothing and is only held, for the task and the features to read

``Decoder`` keeps ``held``, ``prev``, ``age``, ``primed`` and ``seen`` and states the hold: an unprimed plant (never stepped, cleared, or
whose episode index differs from the one seen) starts at age 0; a plant latches where ``age % K == 0`` -- ``prev = held`` (unprimed: the
new y), ``held = y`` -- and otherwise applies ``held`` again.  The device gives these bits exactly.

Order rules (``env.set_control_orders``, npb_set_control_orders, nuclear_sim_amd/csrc/npd_control_orders.h): a rule reads the held value
of a "value" axis and orders one service where it is above the rule's threshold.  A rule is ``{"axis", "family": "pump" | "component" |
"turbine", "action": the family's catalog index, "unit", "option", "amount", "threshold", "min_interval"}`` (``_lib.control_orders_request``
makes them from the caller's words).  ``Orders`` keeps ``since`` and states which plants fire: with ``latch`` "the decode read the plant's
row on this step" and ``restart`` "it found the plant unprimed" (``Decoder.step`` returns both), for r ascending ``c = NEVER if restart
else since[r]``, ``fire = latch and held[axis_r] > threshold_r and (c == NEVER or c >= min_interval_r)``, ``since[r] = 1 if fire else
(NEVER if c == NEVER else c + 1)``, saturating below NEVER.  What a firing plant gets is the family's ``perform_*`` call
(``Orders.calls``), rule by rule."""
from typing import Dict, Optional

import numpy as np

AXES_MAX = 8             # include/npb.h NPB_CONTROLS_AXES_MAX
INTERVAL_MAX = 64        # NPB_CONTROLS_INTERVAL_MAX
KINDS = ("rate", "target", "column", "value")      # NPB_CONTROL_KIND_*, in order
ACTUATORS = ("rod", "flow", "valve", "boron")      # NPB_ACTUATOR_*, in order
INPUTS = ("power_setpoint", "cooling_water_temp")      # NPB_CONTROL_INPUT_*, in order
DTYPES = ("float32", "float64")      # NPB_CONTROLS_F32, NPB_CONTROLS_F64
MEMBERS = {"rod": "prim.control_rod_position", "flow": "prim.coolant_flow_rate", "valve": "prim.steam_valve_position",
           "boron": "prim.boron_concentration"}
UP_CODES = {"rod": 1, "flow": 2, "valve": 4, "boron": 10}      # the increasing ControlAction code of each actuator
DOWN_CODES = {"rod": 0, "flow": 3, "valve": 5, "boron": 9}     # the decreasing one
RANGES = {"rod": (0.0, 100.0), "flow": (5000.0, 50000.0), "valve": (0.0, 100.0), "boron": (0.0, 3000.0)}
# npb_params_default: max_control_rod_speed, max_flow_change_rate, max_valve_speed; boron's 50.0 is a literal of the reference
DEFAULT_SPEEDS = {"rod": 5.0, "flow": 1000.0, "valve": 10.0, "boron": 50.0}
ORDERS_MAX = 8           # NPB_CONTROL_ORDERS_MAX
NEVER = 0x7fffffff       # NPB_CONTROL_ORDER_NEVER: the rule has not fired since the plant's restart
FAMILIES = ("pump", "component", "turbine")      # NPB_ORDER_*, in order
MODES = ("full", "primary_sg", "primary")        # NPB_MODE_*, in order

# the branch report, one word per axis and plant
LATCHED, HELD, UNPRIMED, NAN_IN, CLIP_LO, CLIP_HI, DEADBAND = 1, 2, 4, 8, 16, 32, 64
RATE_UP, RATE_DOWN, RATE_ZERO, LIMIT_HI, LIMIT_LO = 128, 256, 512, 1024, 2048
TARGET_REACHED, TARGET_NOT_REACHED, TARGET_EQUAL, TARGET_OUT_OF_RANGE, COLUMN, VALUE = 4096, 8192, 16384, 32768, 65536, 131072
BRANCHES = {"LATCHED": LATCHED, "HELD": HELD, "UNPRIMED": UNPRIMED, "NAN_IN": NAN_IN, "CLIP_LO": CLIP_LO, "CLIP_HI": CLIP_HI, "DEADBAND": DEADBAND,
            "RATE_UP": RATE_UP, "RATE_DOWN": RATE_DOWN, "RATE_ZERO": RATE_ZERO, "LIMIT_HI": LIMIT_HI, "LIMIT_LO": LIMIT_LO,
            "TARGET_REACHED": TARGET_REACHED, "TARGET_NOT_REACHED": TARGET_NOT_REACHED, "TARGET_EQUAL": TARGET_EQUAL,
            "TARGET_OUT_OF_RANGE": TARGET_OUT_OF_RANGE, "COLUMN": COLUMN, "VALUE": VALUE}


def axis(kind: str, target: str, scale: float = 1.0, offset: float = 0.0, lo: Optional[float] = None, hi: Optional[float] = None,
         nan_to: float = 0.0, deadband: float = 0.0, max_magnitude: float = 1.0) -> Dict:
    """one axis of a spec, with the defaults: a rate is clipped to [-1, 1], a target or a column is not clipped"""
    if lo is None:
        lo = -1.0 if kind == "rate" else -np.inf
    if hi is None:
        hi = 1.0 if kind == "rate" else np.inf
    return {"kind": kind, "target": target, "scale": float(scale), "offset": float(offset), "lo": float(lo), "hi": float(hi),
            "nan_to": float(nan_to), "deadband": float(deadband), "max_magnitude": float(max_magnitude)}


def check(spec: Dict) -> None:
    """ValueError, naming the reason, for a spec the device would refuse (npb_controls_check) as far as the host words show it"""
    axes, K = list(spec["axes"]), spec["interval"]
    if not 1 <= len(axes) <= AXES_MAX:
        raise ValueError("controls take 1 to %d axes, not %d" % (AXES_MAX, len(axes)))
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= INTERVAL_MAX:
        raise ValueError("the interval must be 1 .. %d, not %r" % (INTERVAL_MAX, K))
    if spec.get("dtype", "float32") not in DTYPES:
        raise ValueError("the input type must be float32 or float64 (no half types), not %r" % (spec.get("dtype"),))
    taken = set()
    for a, D in enumerate(axes):
        if D["kind"] not in KINDS:
            raise ValueError("axis %d: unknown kind %r: one of %r" % (a, D["kind"], KINDS))
        names = INPUTS if D["kind"] == "column" else ACTUATORS if D["kind"] != "value" else (None,)
        if D["target"] not in names:
            raise ValueError("axis %d: unknown %s %r: one of %r" % (a, "input" if D["kind"] == "column" else "actuator", D["target"], names))
        if D["target"] is not None and D["target"] in taken:
            raise ValueError("axis %d: %r is already moved by another axis" % (a, D["target"]))
        taken.add(D["target"])
        for name in ("scale", "offset", "nan_to", "deadband", "max_magnitude"):
            if not np.isfinite(float(D[name])):
                raise ValueError("axis %d: %s must be finite, not %r" % (a, name, D[name]))
        for name in ("deadband", "max_magnitude"):
            if D[name] < 0:
                raise ValueError("axis %d: a negative %s" % (a, name))
        if np.isnan(float(D["lo"])) or np.isnan(float(D["hi"])):
            raise ValueError("axis %d: a NaN clip limit" % a)
        if D["lo"] > D["hi"]:
            raise ValueError("axis %d: a clip with lo > hi" % a)


def transform(D: Dict, x: np.ndarray):
    """(y, report) of one axis over the elements ``x``: the statement's transform in its order, and which of its branches each took"""
    x = np.asarray(x).astype(np.float64)
    report = np.zeros(x.shape, dtype=np.uint32)
    with np.errstate(all="ignore"):
        nan = np.isnan(x)
        report[nan] |= NAN_IN
        x = np.where(nan, np.float64(D["nan_to"]), x)
        scaled = x * np.float64(D["scale"])
        y = scaled + np.float64(D["offset"])
        low = y < D["lo"]
        report[low] |= CLIP_LO
        y = np.where(low, np.float64(D["lo"]), y)
        high = y > D["hi"]
        report[high] |= CLIP_HI
        y = np.where(high, np.float64(D["hi"]), y)
        if D["kind"] == "rate":
            dead = np.abs(y) < D["deadband"]
            report[dead] |= DEADBAND
            y = np.where(dead, 0.0, y)
    return y, report


def move(actuator: str, up: bool, pos: np.ndarray, mag, speed: float, dt: float):
    """(new position, clamped) -- what the reference's _apply_control_actions makes of ``pos`` with the actuator's increasing (``up``) or
    decreasing code at magnitude ``mag``: Python's max / min against the range limit, the rate ``speed * dt * mag`` in that order"""
    lo, hi = RANGES[actuator]
    step = np.float64(speed) * np.float64(dt) * mag
    with np.errstate(all="ignore"):
        if up:
            raw = pos + step
            return np.where(raw < hi, raw, hi), raw > hi      # min(hi, raw) keeps hi unless raw is strictly smaller
        raw = pos - step
        return np.where(raw > lo, raw, lo), raw < lo


class Decoder:
    """The hold and the decode of ``n`` plants.  ``speeds``: ``{"rod": max_control_rod_speed, "flow": max_flow_change_rate, "valve":
    max_valve_speed}`` (defaults: the library's); ``storage``: the handle's storage type -- under "float32" a moved member is rounded to
    float32, as the device rounds it at its store."""

    def __init__(self, spec: Dict, n: int, dt: float = 1.0, speeds: Optional[Dict] = None, storage: str = "float64"):
        check(spec)
        self.spec, self.n, self.dt, self.storage = spec, int(n), float(dt), storage
        self.speeds = dict(DEFAULT_SPEEDS, **(speeds or {}))
        A = len(spec["axes"])
        self.held = np.zeros((A, self.n))
        self.prev = np.zeros((A, self.n))
        self.age = np.zeros(self.n, dtype=np.int32)
        self.primed = np.zeros(self.n, dtype=np.int32)
        self.seen = np.zeros(self.n, dtype=np.int32)

    def clear(self, mask=None) -> None:
        """the masked plants (None = all) unprimed"""
        if mask is None:
            self.primed[:] = 0
        else:
            self.primed[np.asarray(mask).astype(bool)] = 0

    def state(self) -> Dict[str, np.ndarray]:
        return {name: getattr(self, name).copy() for name in ("held", "prev", "age", "primed", "seen")}

    def load_state(self, state) -> None:
        for name in ("held", "prev", "age", "primed", "seen"):
            getattr(self, name)[...] = state[name]

    def step(self, x, members: Dict[str, np.ndarray], index=None) -> Dict:
        """One step.  ``x``: the policy's output [n, A]; ``members``: the position of every actuator an axis names, [n] each, by the names
        of ``ACTUATORS``; ``index``: the carried episode indices or None.  Returns {"members": the new positions of those actuators,
        "columns": {input: [n]} of the column axes, "held", "prev": [A, n] (the Decoder's own arrays), "report": uint32 [A, n], the
        branches of ``BRANCHES`` each axis took on each plant}."""
        x = np.asarray(x).reshape(self.n, len(self.spec["axes"]))
        K = self.spec["interval"]
        seen = self.seen if index is None else np.asarray(index, dtype=np.int32)
        primed = (self.primed != 0) & (seen == self.seen)
        age = np.where(primed, self.age, 0).astype(np.int32)
        latch = age % K == 0
        new, columns = {}, {}
        report = np.zeros((len(self.spec["axes"]), self.n), dtype=np.uint32)
        for a, D in enumerate(self.spec["axes"]):
            y_new, rep = transform(D, x[:, a])
            rep = np.where(latch, rep | LATCHED, HELD).astype(np.uint32)
            rep[~primed] |= UNPRIMED
            y = np.where(latch, y_new, self.held[a])
            self.prev[a] = np.where(latch, np.where(primed, self.held[a], y_new), self.prev[a])
            self.held[a] = y
            if D["kind"] in ("column", "value"):
                if D["kind"] == "column":
                    columns[D["target"]] = y.copy()
                rep |= COLUMN if D["kind"] == "column" else VALUE
                report[a] = rep
                continue
            t = D["target"]
            pos = np.asarray(members[t], dtype=np.float64)
            speed = self.speeds[t]
            moved = pos.copy()
            with np.errstate(all="ignore"):
                if D["kind"] == "rate":
                    up, hit_hi = move(t, True, pos, y, speed, self.dt)
                    down, hit_lo = move(t, False, pos, -y, speed, self.dt)
                    moved = np.where(y > 0, up, np.where(y < 0, down, pos))
                    rep[y > 0] |= RATE_UP
                    rep[y < 0] |= RATE_DOWN
                    rep[~(y > 0) & ~(y < 0)] |= RATE_ZERO
                    rep[(y > 0) & hit_hi] |= LIMIT_HI
                    rep[(y < 0) & hit_lo] |= LIMIT_LO
                else:
                    up, hit_hi = move(t, True, pos, np.float64(D["max_magnitude"]), speed, self.dt)
                    down, hit_lo = move(t, False, pos, np.float64(D["max_magnitude"]), speed, self.dt)
                    above, below = y > pos, y < pos
                    to_up = np.where(y < up, y, up)           # min(up, y)
                    to_down = np.where(y > down, y, down)     # max(down, y)
                    moved = np.where(above, to_up, np.where(below, to_down, pos))
                    lo, hi = RANGES[t]
                    outside = (above & (y > hi) & hit_hi) | (below & (y < lo) & hit_lo)
                    reached = (above | below) & (moved == y)
                    rep[reached] |= TARGET_REACHED
                    rep[(above | below) & ~reached & ~outside] |= TARGET_NOT_REACHED
                    rep[outside] |= TARGET_OUT_OF_RANGE
                    rep[~above & ~below] |= TARGET_EQUAL
            if self.storage == "float32":
                moved = moved.astype(np.float32).astype(np.float64)
            new[t] = moved
            report[a] = rep
        self.age = (age + 1).astype(np.int32)
        self.primed[:] = 1
        self.seen = seen.copy()
        return {"members": new, "columns": columns, "held": self.held, "prev": self.prev, "report": report, "latch": latch, "restart": ~primed}


def orders_check(rules, spec: Dict, n_plants: int = 1, mode: str = "full") -> None:
    """ValueError, naming the reason, for order rules the device would refuse (npb_control_orders_check): ``spec`` the controls' spec,
    ``mode`` the handle's"""
    from . import _lib
    rules = list(rules)
    if n_plants < 1:
        raise ValueError("n_plants must be >= 1")
    if spec is None:
        raise ValueError("order rules need controls: set_controls() first")
    if mode not in MODES:
        raise ValueError("unknown mode %r: one of %r" % (mode, MODES))
    if not 1 <= len(rules) <= ORDERS_MAX:
        raise ValueError("order rules: 1 to %d, not %d" % (ORDERS_MAX, len(rules)))
    axes = spec["axes"]
    for r, R in enumerate(rules):
        where = "order rule %d" % r
        a, unit = R["axis"], R["unit"]
        if not 0 <= a < len(axes):
            raise ValueError("%s: axis %r: the controls' axes are 0 .. %d" % (where, a, len(axes) - 1))
        if axes[a]["kind"] != "value":
            raise ValueError("%s: axis %d is a %r axis: a rule reads a 'value' axis" % (where, a, axes[a]["kind"]))
        if R["family"] == "pump":
            if not 0 <= R["action"] < len(_lib.MAINT_ACTION_NAMES):
                raise ValueError("%s: pump action %r is outside the catalog" % (where, R["action"]))
            if not _lib.MAINT_ACTION_HANDLERS[R["action"]]:
                raise ValueError("%s: pump action %r has no handler" % (where, _lib.MAINT_ACTION_NAMES[R["action"]]))
            if not 0 <= unit < len(_lib.PUMP_IDS):
                raise ValueError("%s: feedwater pump %r does not exist (0 .. 3)" % (where, unit))
            if R["action"] == _lib.MAINT_BEARING_REPLACEMENT and not 0 <= R["option"] <= 3:
                raise ValueError("%s: bearing %r is outside its range (0 .. 3)" % (where, R["option"]))
        elif R["family"] == "component":
            if not 0 <= R["action"] < len(_lib.COMPONENT_ACTIONS):
                raise ValueError("%s: component action %r is outside the catalog" % (where, R["action"]))
            kind = _lib.COMPONENT_ACTIONS[R["action"]][0]
            if kind in ("steam_generator", "ejector") and not 0 <= unit < _lib.COMPONENT_UNITS[kind]:
                raise ValueError("%s: %s %r does not exist (0 .. %d)" % (where, kind, unit, _lib.COMPONENT_UNITS[kind] - 1))
            if not (mode == "full" or (mode == "primary_sg" and kind in ("steam_generator", "steam_generator_system"))):
                raise ValueError("%s: the %r mode does not step the %s" % (where, mode, kind))
        elif R["family"] == "turbine":
            if not 0 <= R["action"] < len(_lib.TURBINE_ACTIONS):
                raise ValueError("%s: turbine action %r is outside the catalog" % (where, R["action"]))
            kind = _lib.TURBINE_ACTIONS[R["action"]][0]
            if kind in ("bearing", "stage") and not 0 <= unit < _lib.TURBINE_UNITS[kind]:
                raise ValueError("%s: turbine %s %r does not exist (0 .. %d)" % (where, kind, unit, _lib.TURBINE_UNITS[kind] - 1))
            if R["action"] == _lib.TURBINE_THRUST_ADJUSTMENT and unit != _lib.TURBINE_THRUST_BEARING:
                raise ValueError("%s: a thrust adjustment on journal bearing %r (the thrust bearing is %d)" % (where, unit, _lib.TURBINE_THRUST_BEARING))
            if mode != "full":
                raise ValueError("%s: the %r mode does not step the turbine" % (where, mode))
        else:
            raise ValueError("%s: unknown family %r: one of %r" % (where, R["family"], FAMILIES))
        if not np.isfinite(float(R["threshold"])) or not np.isfinite(float(R["amount"])):
            raise ValueError("%s: the threshold and the amount must be finite" % where)
        K = R["min_interval"]
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1 or K > NEVER:
            raise ValueError("%s: min_interval must be an int >= 1, not %r" % (where, K))


class Orders:
    """The order rules of ``n`` plants: which rule fires on which plant, step by step, and the ``perform_*`` calls that are its effect"""

    def __init__(self, rules, spec: Dict, n: int, mode: str = "full"):
        orders_check(rules, spec, n, mode)
        self.rules, self.n = [dict(R) for R in rules], int(n)
        self.since = np.full((len(self.rules), self.n), NEVER, dtype=np.int32)

    def state(self) -> Dict[str, np.ndarray]:
        return {"since": self.since.copy()}

    def load_state(self, state) -> None:
        self.since[...] = state["since"]

    def step(self, held, latch, restart) -> np.ndarray:
        """One step behind the decode.  ``held``: the Decoder's [A, n]; ``latch`` / ``restart``: bool [n] of ``Decoder.step``.  Returns
        ``fire`` bool [R, n] and keeps ``since``"""
        held, latch, restart = np.asarray(held, dtype=np.float64), np.asarray(latch, dtype=bool), np.asarray(restart, dtype=bool)
        fire = np.zeros((len(self.rules), self.n), dtype=bool)
        for r, R in enumerate(self.rules):
            c = np.where(restart, NEVER, self.since[r]).astype(np.int64)
            with np.errstate(invalid="ignore"):
                above = held[R["axis"]] > R["threshold"]
            fire[r] = latch & above & ((c == NEVER) | (c >= R["min_interval"]))
            self.since[r] = np.where(fire[r], 1, np.where(c >= NEVER - 1, c, c + 1)).astype(np.int32)
        return fire

    def calls(self, fire):
        """the equivalent ``BatchedPlantEnv.perform_*`` calls of one step, in order: [(method name, kwargs)], rule r's masked by ``fire[r]``"""
        from . import _lib
        out = []
        for r, R in enumerate(self.rules):
            mask = np.asarray(fire[r]).astype(np.uint8)
            if R["family"] == "pump":
                out.append(("perform_maintenance", {"action": R["action"], "pump": R["unit"], "mask": mask, "bearing": R["option"],
                                                    "target_level": R["amount"]}))
            elif R["family"] == "component":
                out.append(("perform_component_maintenance", {"component": _lib.COMPONENT_ACTIONS[R["action"]][0], "action": R["action"],
                                                              "unit": R["unit"], "mask": mask, "cleaning_type": R["option"],
                                                              "tubes_to_plug": R["amount"]}))
            else:
                out.append(("perform_turbine_maintenance", {"component": _lib.TURBINE_ACTIONS[R["action"]][0], "action": R["action"],
                                                            "unit": R["unit"], "mask": mask}))
        return out
