"""GPU: the order rules (npb_set_control_orders, npd_control_orders.h) over EVERY order the check accepts, on a segmented arena, at ragged
sizes, in the primary_sg mode, at time's edges, and with every reader of the maintenance log on the same handle.

npd_order_apply states a second time which sections an action touches, beside the three operator kernels.  The sweep fires each of the
186 accepted orders (control_orders_support.order_table, enumerated from the catalogs) and the option variants, eight rules at a time,
against the TWIN of tests/test_control_orders_gpu.py: env A has the rules, env B the same controls and the perform_* calls that
controls.Orders states, env C the controls only.  A and B are compared by bits in the outputs and the whole state, A's fired and since
with the statement, the drained logs record by record.  Every comparison in this file is by bits; there is no tolerance.

NO_EFFECT keeps the sweep from proving nothing: an order after which B's plants equal C's in every bit of state would pass with a kernel
that skipped it.  The set is measured on B and C -- the operator kernels and the step, never on A -- and held as a literal: the orders
found without effect must be exactly these."""
import ctypes

import numpy as np
import pytest
import torch

import control_orders_support as cos
from control_orders_support import (AXES, DT, NEVER, RULES, _compare_envs, _decoder, _follow, _inputs, _loop_env, _make, _np, _positions,
                                    _records, _same_np, _tbits)

pytestmark = pytest.mark.gpu

LIFE_RULES = [RULES[0], RULES[6], (3, "lubrication", "turbine_oil_change", {"min_interval": 4})]      # min_interval 1, 5 and 4
SWEEP = cos.order_table() + cos.option_variants()
GROUPS = cos.groups(SWEEP)
CHUNKS = 4

# The orders whose handler moves no carried member in the swept start state, or only members the step assigns anew before anything reads
# them ("Order rules", names each with its reason).  Measured on B against C; see the head of this file.
_UNITS = {"pump": 4, "steam_generator": 3, "ejector": 2, "bearing": 4}
NO_EFFECT = set()
for _component, _names in (("pump", ("vibration_analysis", "oil_analysis")),
                           ("steam_generator", ("tube_bundle_inspection", "water_chemistry_adjustment", "tsp_inspection", "tsp_flow_test",
                                                "tube_interior_inspection", "tube_interior_eddy_current_testing", "primary_chemistry_optimization",
                                                "tube_eddy_current_testing")),
                           ("ejector", ("vacuum_ejector_inspection",)),
                           ("bearing", ("turbine_bearing_inspection", "bearing_clearance_check", "bearing_alignment"))):
    NO_EFFECT |= {"%s/%s/%d" % (_component, _name, _u) for _name in _names for _u in range(_UNITS[_component])}
NO_EFFECT |= {"condenser/vacuum_system_test/0", "turbine/turbine_performance_test/0", "turbine/thermal_stress_analysis/0"}
# what only the step's own assignments overwrite: the system's availability flag, the lubrication effectiveness, the metal temperature of
# bearing 3 (the only bearing whose temperature feeds no lubrication wear rate)
NO_EFFECT |= {"steam_generator_system/system_coordination_maintenance/0", "turbine/turbine_system_optimization/0",
              "lubrication/lubrication_system_test/0", "bearing/routine_maintenance/3", "bearing/turbine_oil_change/3"}
# SteamJetEjector.perform_cleaning has no hydroblast branch: the option variant writes nothing
NO_EFFECT |= {"ejector/vacuum_ejector_cleaning/0/cleaning_type=3"}


def _same_t(a, b, where):
    assert a.shape == b.shape and a.dtype == b.dtype, (where, a.shape, b.shape)
    assert torch.equal(_tbits(a), _tbits(b)), where


def _same_columns(got, want, where):
    """two drained column dicts (event windows, episode records): the same names, every column by bits"""
    from nuclear_sim_amd import eventwin
    assert sorted(got) == sorted(want), (where, sorted(got), sorted(want))
    eventwin.same(got, want)


def _twin_step(A, B, dec, orders, x, t, index=None):
    """one step of the twin: B gets the statement's perform_* calls, then both step; outputs, state, fired and since by bits.  Returns
    (fire, A's step outputs, B's step outputs)"""
    out = dec.step(x, _positions(B), index)
    fire = orders.step(out["held"], out["latch"], out["restart"])
    for name, kw in orders.calls(fire):
        ok = getattr(B, name)(**kw)
        assert np.array_equal(_np(ok) != 0, kw["mask"] != 0), (t, name)      # at run time fire means success
    rb = B.step(controls=torch.as_tensor(x))
    _same_np(B.controls_state()["held"], out["held"], ("the twin's held", t))
    ra = A.step(controls=torch.as_tensor(x))
    _compare_envs(A, ra, B, rb, t)
    got = A.control_orders()
    _same_np(got["fired"], fire.astype(np.float64), ("fired", t))
    assert torch.equal(ra[3]["orders"], got["fired"]) and "orders" not in rb[3]
    assert np.array_equal(got["since"], orders.since), ("since", t, np.argwhere(got["since"] != orders.since)[:4].tolist())
    return fire, ra, rb


# ---------------------------------------------------------------------------------------------------------------- 1. the order table
@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_every_accepted_order_is_the_perform_call_by_bits(chunk, storage):
    """a quarter of the groups: per group the swept members poked anew on A, B and C (C's whole state B's first, so that what differs
    behind the step is this group's), the group's rules set on A, one step"""
    n = cos.SWEEP_N
    per = (len(GROUPS) + CHUNKS - 1) // CHUNKS
    mine = GROUPS[chunk * per:(chunk + 1) * per]
    A, B, C = (_make(n, storage=storage, maintenance_log=8192) for _ in range(3))
    for e in (A, B, C):
        e.set_controls(cos.SWEEP_AXES, interval=1)
    pokes = [(name, instance, k, torch.as_tensor(v, device=A.device)) for name, instance, k, v in cos.sweep_pokes(n)]
    dec = _decoder(B, storage)
    p = np.arange(n)
    quiet_wave = slice(64, 128)
    found, fired_total = set(), 0
    for g, group in enumerate(mine):
        C.load_state_arrays(*B.state_arrays())
        for name, instance, k, v in pokes:
            for e in (A, B, C):
                e.set_field(name, v, instance, k)
        A.set_control_orders(cos.group_rules(group))
        orders = A.control_orders_spec()
        assert (A.control_orders_state()["since"] == NEVER).all()
        x, want = cos.sweep_inputs(len(group), n)
        fire, ra, rb = _twin_step(A, B, dec, orders, x, (chunk, g))
        assert np.array_equal(fire, want), (chunk, g)
        fired_total += int(fire.sum())
        rc = C.step(controls=torch.as_tensor(x))
        (fa, ia), (fb, ib), (fc, ic) = A.state_arrays(), B.state_arrays(), C.state_arrays()
        # the wave in which nothing fires left before the arena was touched: C's plants, in state and outputs
        assert torch.equal(_tbits(fa[:, quiet_wave]), _tbits(fc[:, quiet_wave])) and torch.equal(ia[:, quiet_wave], ic[:, quiet_wave]), (chunk, g)
        for k, (u, v) in enumerate(zip(ra[:3], rc[:3])):
            assert torch.equal(_tbits(u[quiet_wave]), _tbits(v[quiet_wave])), (chunk, g, k)
        # which orders leave nothing behind the step: B against C on the plants that fired the rule alone
        for r, order in enumerate(group):
            alone = torch.as_tensor((p < 64) & (p % 8 == r), device=fb.device)
            if torch.equal(_tbits(fb[:, alone]), _tbits(fc[:, alone])) and torch.equal(ib[:, alone], ic[:, alone]):
                found.add(cos.label(order))
    labels = {cos.label(o) for group in mine for o in group}
    print("chunk %d %s: %d orders in %d groups, %d firings, %d without effect" % (chunk, storage, len(labels), len(mine), fired_total, len(found)))
    assert found == NO_EFFECT & labels, (sorted(found - NO_EFFECT), sorted((NO_EFFECT & labels) - found))
    (got, kinds), (want_rec, _k), (plain, plain_kinds) = _records(A), _records(B), _records(C)
    assert got == want_rec and got != plain
    assert sum(kinds.get(k, 0) for k in (2, 3, 4)) == fired_total and not {2, 3, 4} & set(plain_kinds)
    # an ignored unit that is not 0: the records are the twin's (above), whose kernel sets an ignored unit to 0 before it logs, as
    # npb_set_control_orders does to the rule
    from nuclear_sim_amd import _lib, maintlog
    i_kind, i_action, i_unit = (maintlog.EVENT_DTYPE.names.index(f) for f in ("kind", "action", "pump"))
    for component, name, opt in (o for group in mine for o in group):
        if component in cos.IGNORED_UNIT and opt["unit"] != 0:
            catalog, kind = (_lib.COMPONENT_ACTIONS, 3) if component in _lib.COMPONENT_KINDS else (_lib.TURBINE_ACTIONS, 4)
            units = [r[i_unit] for r in want_rec if (r[i_kind], r[i_action]) == (kind, catalog.index((component, name)))]
            assert units == [0] * 10, (component, name, opt, units)      # 8 plants alone, 2 with every rule; the twin's kernel logs unit 0
    for e in (A, B, C):
        e.close()


def test_the_no_effect_orders_are_a_subset_of_the_table():
    assert NO_EFFECT <= {cos.label(o) for o in SWEEP} and len(NO_EFFECT) == 8 + 24 + 2 + 12 + 3 + 5 + 1


# ---------------------------------------------------------------------------------------------------------------- 2. segments and ragged sizes
def _segment_firing(n):
    """plants 0, 63, 64, 127, 192, 255 and a pseudo-random third of segments 0, 1 and 3; segment 2 (128 .. 191) quiet throughout"""
    rng = np.random.default_rng(64)
    firing = rng.random(n) < 1.0 / 3.0
    firing[[0, 63, 64, 127, 192, 255]] = True
    firing[128:192] = False
    return firing


def _segment_run(monkeypatch, seg, storage, steps=6):
    n = 256
    monkeypatch.setenv("NPB_ARENA_SEGMENT", str(seg))
    A, B = (_make(n, storage=storage, maintenance_log=16384) for _ in range(2))
    for e in (A, B):
        assert int(e.L.npb_state_arena_segment(e._h)) == seg
        cos._poke(e)
        e.set_controls(AXES, interval=1)
    A.set_control_orders(RULES)
    orders, dec, rng = A.control_orders_spec(), _decoder(B, storage), np.random.default_rng(256)
    firing = _segment_firing(n)
    corners = np.array([0, 63, 64, 127, 192, 255])
    per_segment = np.zeros((len(RULES), 4), dtype=int)
    trace = []
    for t in range(steps):
        x = _inputs(t, n, rng, np.float32, quiet=~firing)
        x[corners, 2:] = np.abs(x[corners, 2:]) + 0.8      # the corner plants of the segments fire whenever their interval allows
        fire, ra, _rb = _twin_step(A, B, dec, orders, x, (seg, t))
        assert not fire[:, ~firing].any()
        per_segment += fire.reshape(len(RULES), 4, 64).sum(axis=2)
        f, i = A.state_arrays()
        trace.append((f, i, ra[0].clone(), ra[1].clone(), ra[2].clone(), ra[3]["orders"].clone(), torch.as_tensor(A.control_orders()["since"])))
    assert fire[:, corners].any() and (per_segment[:, 2] == 0).all()
    assert ((per_segment > 0).sum(axis=1) >= 2).all(), per_segment      # every rule fired in at least two segments
    (got, _kinds), (want, _k) = _records(A), _records(B)
    assert got == want
    A.close(); B.close()
    return trace, got


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_segmented_arena_against_the_twin_and_against_one_block(monkeypatch, storage):
    """n = 256 with NPB_ARENA_SEGMENT=64: a wave per segment, segment 2 leaving before NPD_SEGMENT; against the twin of the same layout
    and against the run in one block"""
    seg_trace, seg_records = _segment_run(monkeypatch, 64, storage)
    one_trace, one_records = _segment_run(monkeypatch, 0, storage)
    for t, (x, y) in enumerate(zip(seg_trace, one_trace)):
        for k, (u, v) in enumerate(zip(x, y)):
            _same_t(u, v, (t, k))
    assert seg_records == one_records


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_ragged_sizes_against_the_twin(n):
    A, B = (_make(n, maintenance_log=4096) for _ in range(2))
    for e in (A, B):
        cos._poke(e)
        e.set_controls(AXES, interval=1)
    A.set_control_orders(RULES)
    orders, dec, rng = A.control_orders_spec(), _decoder(B, "f64"), np.random.default_rng(n)
    quiet = np.arange(n) % 5 == 4      # (plant 0 orders: n = 1 has a plant that fires)
    fired = np.zeros(len(RULES), dtype=int)
    for t in range(4):
        x = _inputs(t, n, rng, np.float32, quiet=quiet)
        x[0, 2:] = 0.875 + 0.0625 * t
        fire, _ra, _rb = _twin_step(A, B, dec, orders, x, (n, t))
        fired += fire.sum(axis=1)
    assert (fired > 0).all(), fired
    assert _records(A)[0] == _records(B)[0]
    A.close(); B.close()


# ---------------------------------------------------------------------------------------------------------------- 3. the primary_sg mode
SG_RULES = [(2, "pump", "oil_top_off", {"unit": 2, "threshold": 0.25, "target_level": 91.5}),
            (3, "steam_generator", "tsp_mechanical_cleaning", {"unit": 0, "threshold": 0.0}),
            (2, "steam_generator_system", "routine_maintenance", {"threshold": 0.5, "min_interval": 2}),      # the three generators in turn
            (3, "steam_generator_system", "system_coordination_maintenance", {"threshold": 0.5, "min_interval": 3}),      # the system's flags alone
            (3, "steam_generator", "primary_scale_cleaning", {"unit": 2, "cleaning_type": "mechanical", "threshold": -0.25})]


def _raw_refusal(env, family, action, unit=0):
    """npb_set_control_orders' own answer to one rule on axis 2, past the Python layer"""
    from nuclear_sim_amd import _lib
    table = (_lib.NpbControlOrder * 1)()
    table[0].axis, table[0].family, table[0].action, table[0].unit, table[0].min_interval, table[0].amount = 2, _lib.ORDER_FAMILIES[family], action, unit, 1, 0.0
    fired = torch.zeros((1, env.n), dtype=torch.float64, device=env.device)
    d = _lib.NpbControlOrdersDesc()
    d.n_orders, d.orders, d.fired = 1, table, fired.data_ptr()
    assert env.L.npb_set_control_orders(env._h, ctypes.byref(d)) != 0
    return env.L.npb_last_error(env._h).decode()


def test_primary_sg_mode_against_the_twin_and_its_refusals():
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 130
    A, B = (BatchedPlantEnv(n, dt=DT, heat_source="reactor", mode="primary_sg", maintenance=True) for _ in range(2))
    for e in (A, B):
        e.enable_maintenance_log(8192)
        for name, instance, k, v in cos.sweep_pokes(n):
            if name.split(".")[0] in ("pump", "sg", "sec"):
                e.set_field(name, v, instance, k)
        e.set_controls(AXES, interval=1)
    A.set_control_orders(SG_RULES)
    # what the mode does not step is refused: by the Python check with its words, by the library with its own; what was set stays
    with pytest.raises(ValueError, match="the 'primary_sg' mode does not step the condenser"):
        A.set_control_orders([(2, "condenser", "condenser_tube_cleaning")])
    with pytest.raises(ValueError, match="the 'primary_sg' mode does not step the turbine"):
        A.set_control_orders([(2, "stage", "overhaul", {"unit": 3})])
    assert "a component the mode does not step" in _raw_refusal(A, "component", _lib.COMPONENT_ACTIONS.index(("condenser", "condenser_tube_cleaning")))
    assert "a component the mode does not step" in _raw_refusal(A, "component", _lib.COMPONENT_ACTIONS.index(("ejector", "general")), 1)
    assert "a turbine rule in a mode that steps no turbine" in _raw_refusal(A, "turbine", _lib.TURBINE_ACTIONS.index(("turbine", "vibration_analysis")))
    orders, dec, rng = A.control_orders_spec(), _decoder(B, "f64"), np.random.default_rng(3)
    assert len(orders.rules) == len(SG_RULES)
    fired = np.zeros(len(SG_RULES), dtype=int)
    for t in range(6):
        x = _inputs(t, n, rng, np.float32)
        fire, _ra, _rb = _twin_step(A, B, dec, orders, x, t)
        fired += fire.sum(axis=1)
    assert (fired > 0).all(), fired
    (got, kinds), (want, _k) = _records(A), _records(B)
    assert got == want and kinds.get(2, 0) == fired[0] and kinds.get(3, 0) == fired[1:].sum() and 4 not in kinds
    A.close(); B.close()


# ---------------------------------------------------------------------------------------------------------------- 4. time's edges
def test_since_saturates_below_never_on_the_device():
    """since rows holding 1, min_interval - 1, NEVER - 2, NEVER - 1 and NEVER under a rule with min_interval = NEVER and one with 3"""
    n = 70
    env = _make(n)
    env.set_controls(AXES, interval=1)
    rules = [(2, "pump", "oil_analysis", {"unit": 1, "threshold": 0.25, "min_interval": NEVER}),
             (3, "stage", "blade_replacement", {"unit": 4, "threshold": 0.0, "min_interval": 3})]
    env.set_control_orders(rules)
    dec, orders, rng = _decoder(env, "f64"), env.control_orders_spec(), np.random.default_rng(4)
    p = np.arange(n)
    above = p % 10 < 5      # half of the plants above both thresholds, half below
    rows = [np.array([1, K - 1, NEVER - 2, NEVER - 1, NEVER], dtype=np.int64)[p % 5] for K in (NEVER, 3)]
    history = []
    for t in range(4):
        x = _inputs(t, n, rng, np.float32, quiet=~above)
        x[above, 2:] = 0.5 + 0.25 * (t % 2)
        out = dec.step(x, _positions(env))
        if t == 1:      # behind the priming step: a loaded count is read, not restarted
            state = {"since": np.stack(rows).astype(np.int32)}
            env.load_control_orders_state(state)
            orders.load_state(state)
            assert np.array_equal(env.control_orders_state()["since"], state["since"])
        fire = orders.step(out["held"], out["latch"], out["restart"])
        env.step(controls=torch.as_tensor(x))
        got = env.control_orders()
        _same_np(got["fired"], fire.astype(np.float64), ("fired", t))
        assert np.array_equal(got["since"], orders.since), (t, np.argwhere(got["since"] != orders.since)[:4].tolist())
        history.append((fire.copy(), orders.since.copy()))
    # the statement itself, by hand, on the step behind the load: under min_interval = NEVER only a count AT NEVER fires; NEVER - 2 and
    # NEVER - 1 end at NEVER - 1 and stay; under 3 the counts 2 and NEVER - x fire where the value is above
    fire1, since1 = history[1]
    k = p % 5
    assert np.array_equal(fire1[0], above & (k == 4)) and np.array_equal(fire1[1], above & (k >= 2))
    want0 = np.where(fire1[0], 1, np.array([2, NEVER - 1, NEVER - 1, NEVER - 1, NEVER])[k])
    assert np.array_equal(since1[0], want0)
    assert np.array_equal(history[3][1][0][~above], np.array([4, NEVER - 1, NEVER - 1, NEVER - 1, NEVER])[k][~above])
    assert np.array_equal(history[3][1][1][~above], np.array([4, 5, NEVER - 1, NEVER - 1, NEVER])[k][~above])
    env.close()


def test_the_largest_interval_latches_twice_in_66_steps():
    from nuclear_sim_amd import controls
    n = 70
    env = _make(n)
    env.set_controls(AXES, interval=controls.INTERVAL_MAX)
    assert controls.INTERVAL_MAX == 64
    env.set_control_orders(LIFE_RULES)
    dec, orders = _decoder(env, "f64"), env.control_orders_spec()
    _follow(env, dec, orders, 66, np.random.default_rng(64))
    # the rows read on steps 0 and 64 fired; on step 65 every count is 2 or NEVER
    assert sorted(np.unique(orders.since).tolist()) == [2, NEVER] and (orders.since == 2).any(axis=1).all()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the readers of the log
READER_RULES = [(2, "pump", "bearing_replacement", {"unit": 1, "bearing": "pump_bearings", "threshold": 0.25, "min_interval": 2}),
                (3, "steam_generator", "tsp_chemical_cleaning", {"unit": 2, "threshold": 0.0}),
                (3, "stage", "overhaul", {"unit": 7, "threshold": 0.5, "min_interval": 3})]
# one key per catalog matching a rule, one matching the automatic oil_top_off work orders, one that matches nothing
READER_KEYS = [("feedwater", "bearing_replacement", 1), ("component", ("steam_generator", "tsp_chemical_cleaning"), 2),
               ("turbine", ("stage", "overhaul"), 7), "oil_top_off", ("turbine", ("lubrication", "oil_cooler_cleaning"), None)]
TABLES = ("first_created", "first_completed", "n_created", "n_completed")


def _reader_env(n, rules, log, clear_summary=True):
    env = _make(n, autoreset=True, max_episode_steps=5, maintenance_log=16384 if log else None)
    cos._poke(env)
    env.snapshot()
    env.enable_maintenance_summary(READER_KEYS, operator=True)
    env.set_controls(AXES, interval=1)
    if rules:
        env.set_control_orders(READER_RULES)
    env.set_task(reward=[(("completed", 0), 1.0, "delta"), (("completed", 1), 0.5, "delta"), (("completed", 2), 0.25, "delta"),
                         (("work_order", 3), -2.0, "delta"), ("maintenance", -0.125, "delta")], bias=0.5)
    words = [("completed", 0), ("completed", 1), ("completed", 2), ("work_order", 3)]
    env.set_features(words + ([("order", r) for r in range(len(READER_RULES))] if rules else []), stack=2, dtype=torch.float64)
    env.enable_event_windows([("pump.oil_level", 1), ("pump.wear_pump_bearings", 1), ("tstg.stage_deposit_thickness", 0, 7)], triggers=[("completed", 0), ("completed", 2)], pre=1, post=2)
    env.enable_episode_records(clear_summary=clear_summary)
    return env


def _reader_run(log, clear_summary=True, steps=12):
    n = 130
    A, B = _reader_env(n, True, log, clear_summary), _reader_env(n, False, log, clear_summary)
    orders, dec, rng = A.control_orders_spec(), _decoder(B, "f64"), np.random.default_rng(5)
    index = np.zeros(n, dtype=np.int32)
    n_words = 4
    both_folds = 0
    for t in range(steps):
        x = _inputs(t, n, rng, np.float32)
        before = {k: _np(v) for k, v in B.maintenance_summary().items()}
        fire, ra, rb = _twin_step(A, B, dec, orders, x, t, index)
        fa, fb = ra[3]["features"], rb[3]["features"]
        _same_t(fa[:, :, :n_words], fb, ("features", t))
        sa, sb = A.maintenance_summary(), B.maintenance_summary()
        for name in TABLES + ("dropped",):
            _same_t(sa[name], sb[name], (name, t))
        ended = (_np(ra[2]) != 0) | (_np(ra[3]["truncated"]) != 0)
        _same_np(_np(fa[:, -1, n_words:])[~ended], fire.T.astype(np.float64)[~ended], ("the order columns of the newest frame", t))
        assert np.array_equal(_np(ra[3]["episode_index"]), index), t
        # a plant with a rule's record and an automatic record on this step: both folds of the step had something to fold (seen on the
        # tables where the episode went on, so that nothing was cleared behind the folds)
        after = {k: _np(v) for k, v in sa.items()}
        auto = (after["n_created"][3] > before["n_created"][3]) | (after["n_completed"][3] > before["n_completed"][3])
        both_folds += int((auto & fire.any(axis=0) & ~ended).sum())
        index[ended] += 1
    return A, B, both_folds


def test_the_readers_of_the_log_follow_the_rules_as_they_follow_the_perform_calls():
    """summary, episode records that copy and clear it, the task's ("completed", j) / ("work_order", j) / "maintenance" words, the features
    and the event windows on one handle with rules of all three families, against the twin with the same attachments"""
    A, B, both_folds = _reader_run(log=True)
    assert both_folds > 0
    wa, wb = A.event_windows(), B.event_windows()
    _same_columns(wa, wb, "event windows")
    ea, eb = A.episode_records(), B.episode_records()
    _same_columns(ea, eb, "episode records")
    assert len(wa["plant"]) > 0 and len(ea["plant"]) >= 2 * A.n      # episodes ended: 12 steps of episodes of 5
    assert (ea["n_completed"][:, :3].sum(axis=0) > 0).all(), ea["n_completed"].sum(axis=0)      # completions from rules, for every catalog
    assert ea["n_created"][:, 3].sum() > 0 and ea["n_completed"][:, 4].sum() == 0 and ea["n_created"][:, 4].sum() == 0
    assert int(A.maintenance_summary()["dropped"].item()) == 0
    (got, kinds), (want, _k) = _records(A), _records(B)
    assert got == want and {2, 3, 4} <= set(kinds) and kinds.get(0, 0) > 0, kinds
    A.close(); B.close()


def test_the_summary_under_rules_is_the_numpy_fold_of_the_drained_log():
    from nuclear_sim_amd import maintlog
    A, B, both_folds = _reader_run(log=True, clear_summary=False)
    assert both_folds > 0
    tables = {k: _np(v) for k, v in A.maintenance_summary().items()}
    assert int(tables["dropped"]) == 0
    rec = A.maintenance_log_records()
    want = maintlog.summarize(rec, READER_KEYS, A.n, operator=True)
    for name in TABLES:
        g, w = tables[name], want[name]
        assert g.dtype == w.dtype and np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g, w.view(np.int64) if w.dtype == np.float64 else w), name
    assert (want["n_completed"][:3].sum(axis=1) > 0).all() and want["n_created"][3].sum() > 0 and want["n_completed"][4].sum() == 0
    A.close(); B.close()


def test_the_summarys_own_staging_log_under_rules():
    """without a caller's log the summary consumes a staging log of its own at every fold: the tables of A and B by bits at every step"""
    from nuclear_sim_amd._lib import NpbError
    A, B, both_folds = _reader_run(log=False)
    assert both_folds > 0 and int(A.maintenance_summary()["dropped"].item()) == 0
    with pytest.raises(NpbError, match="consumes the log"):
        A.maintenance_log_records()
    ea, eb = A.episode_records(), B.episode_records()
    _same_columns(ea, eb, "episode records")
    assert (ea["n_completed"][:, :3].sum(axis=0) > 0).all() and ea["n_created"][:, 3].sum() > 0
    A.close(); B.close()


def test_a_log_without_the_automatic_maintenance_is_refused_so_the_orders_fold_is_never_the_only_one():
    """the env takes a maintenance log, and with it a summary, only with the automatic maintenance on: a step whose only fold is the one
    behind the orders kernel cannot be set up through it"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv(64, dt=DT)
    with pytest.raises(ValueError, match="needs the automatic maintenance"):
        env.enable_maintenance_log(4096)
    with pytest.raises(ValueError, match="needs the automatic maintenance"):
        env.enable_maintenance_summary(READER_KEYS, operator=True)
    env.close()


def test_collect_is_t_steps_with_the_log_the_summary_a_task_and_episode_records():
    n, T = 70, 8
    keys = [("feedwater", "oil_top_off", 1), ("turbine", ("stage", "overhaul"), 7)]

    def attach(env):
        env.enable_maintenance_log(8192)
        env.enable_maintenance_summary(keys, operator=True)
        env.set_task(reward=[("reward", 1.0), (("completed", 0), -0.5, "delta"), (("completed", 1), -2.0, "delta")], terminate=[("done",)])
        env.enable_episode_records()
    env, twin = _loop_env(n, T, attach, maintenance=True), _loop_env(n, T, attach, maintenance=True)
    got = env.collect(T)
    for t in range(T):
        twin.step()
    want = twin.rollout()
    assert got["t"] == want["t"] == T
    for name in ("obs", "act", "reward", "ended", "episode", "final_row", "final_obs"):
        g, w = got[name], want[name]
        assert (g is None) == (w is None), name
        if g is not None:
            assert torch.equal(_tbits(g), _tbits(w)), name
    (fa, ia), (fb, ib) = env.state_arrays(), twin.state_arrays()
    assert torch.equal(_tbits(fa), _tbits(fb)) and torch.equal(ia, ib)
    assert np.array_equal(env.control_orders()["since"], twin.control_orders()["since"])
    assert torch.equal(env.control_orders()["fired"], twin.control_orders()["fired"])
    sa, sb = env.maintenance_summary(), twin.maintenance_summary()
    for name in TABLES + ("dropped",):
        _same_t(sa[name], sb[name], name)
    ea, eb = env.episode_records(), twin.episode_records()
    _same_columns(ea, eb, "episode records")
    assert len(ea["plant"]) > 0 and (ea["n_completed"].sum(axis=0) > 0).all() and int(sa["dropped"].item()) == 0
    assert _records(env)[0] == _records(twin)[0]
    env.close(); twin.close()
