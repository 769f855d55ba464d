"""CPU: the table of orders that tests/test_control_orders_table_gpu.py sweeps (control_orders_support.order_table) is every order the
request and the check accept, no more and no fewer, and the sweep's firing pattern fires what it is meant to.  No library, no device."""
import numpy as np
import pytest

import control_orders_support as cos
from nuclear_sim_amd import _lib, controls

TABLE = cos.order_table()


def test_the_table_has_the_nine_family_counts_186_in_all():
    counts = {}
    for component, _name, _opt in TABLE:
        counts[component] = counts.get(component, 0) + 1
    assert counts == cos.FAMILY_COUNTS and len(TABLE) == 186
    assert len({cos.label(o) for o in TABLE}) == 186
    assert all(opt == {"unit": 0} for component, _n, opt in TABLE if component in cos.IGNORED_UNIT)


def test_the_table_is_the_brute_force_set_of_accepted_orders_over_units_0_to_14():
    brute = set()
    for component, names, _units in cos.catalog():
        for name in names:
            took = [u for u in range(15) if cos.accepted(component, name, {"unit": u}) is None]
            if component in cos.IGNORED_UNIT:
                assert took == list(range(15)), (component, name)      # ignored: every unit is taken, the table holds unit 0
                took = [0]
            brute |= {(component, name, u) for u in took}
    assert brute == {(component, name, opt["unit"]) for component, name, opt in TABLE}


def test_every_catalog_action_outside_the_table_is_refused_with_its_reason():
    inside = {(component, name, opt["unit"]) for component, name, opt in TABLE}
    refused = {}
    for component, names, units in cos.catalog():
        for name in names:
            for unit in range(units):
                if (component, name, unit) not in inside:
                    refused[(component, name, unit)] = cos.accepted(component, name, {"unit": unit})
    no_handler = [a for a, h in zip(_lib.MAINT_ACTION_NAMES, _lib.MAINT_ACTION_HANDLERS) if not h]
    assert len(no_handler) == 5
    want = {("pump", a, u): "pump action %r has no handler" % a for a in no_handler for u in range(4)}
    want.update({("bearing", "thrust_bearing_adjustment", u): "a thrust adjustment on journal bearing %d (the thrust bearing is 2)" % u for u in (0, 1, 3)})
    assert sorted(refused) == sorted(want)
    for key, reason in want.items():
        assert refused[key] is not None and reason in refused[key], (key, refused[key])
    # the handlers that are not in the catalogs because the device does not offer them keep their own refusal
    for (component, name) in list(_lib.COMPONENT_ACTIONS_NOT_OFFERED) + list(_lib.TURBINE_ACTIONS_NOT_OFFERED):
        assert "is not offered on the device" in cos.accepted(component, name)
    # one past the last unit of every kind that has units
    for component, names, units in cos.catalog():
        if component not in cos.IGNORED_UNIT:
            assert "does not exist" in cos.accepted(component, [n for n in names if (component, n, 0) in inside][0], {"unit": units})


def test_the_option_variants_are_accepted_and_are_what_the_issue_lists():
    V = cos.option_variants()
    assert all(cos.accepted(*o) is None for o in V)
    assert len({cos.label(o) for o in V} | {cos.label(o) for o in TABLE}) == len(V) + 186
    bearings = [o for o in V if o[1] == "bearing_replacement"]
    assert sorted(o[2]["bearing"] for o in bearings) == [1, 2, 3] and len({o[2]["unit"] for o in bearings}) == 1
    for component, name, unit in cos.CLEANING_TYPE_ACTIONS:
        assert sorted(o[2]["cleaning_type"] for o in V if o[:2] == (component, name)) == [1, 2, 3, 4]
        assert {o[2]["unit"] for o in V if o[:2] == (component, name)} == {unit}
    tops = [o[2]["target_level"] for o in V if o[1] == "oil_top_off"]
    levels = {row[1]: row[3] for row in cos.sweep_pokes() if row[0] == "pump.oil_level"}
    assert len(tops) == 2 and 95.0 not in tops
    low = [o for o in V if o[1] == "oil_top_off" and o[2]["target_level"] == min(tops)][0]
    lv = levels[low[2]["unit"]][:64]
    assert (lv > min(tops)).any() and (lv < min(tops)).any()      # below some plants' level, above others'
    assert ("condenser", 3) in {(o[0], o[2]["unit"]) for o in V} and ("lubrication", 2) in {(o[0], o[2]["unit"]) for o in V}
    # the request carries the options where the kernel reads them
    R = _lib.control_orders_request(cos.group_rules(V[:4]))
    assert [D["option"] for D in R[:3]] == [1, 2, 3] and R[3]["option"] == 1 and R[3]["family"] == "component"
    R = _lib.control_orders_request(cos.group_rules([o for o in V if o[1] == "oil_top_off"]))
    assert [D["amount"] for D in R] == tops


def test_the_groups_mostly_share_a_section_and_the_pattern_fires_what_it_is_meant_to():
    G = cos.groups(TABLE + cos.option_variants())
    assert sum(len(g) for g in G) == 186 + len(cos.option_variants()) and all(1 <= len(g) <= 8 for g in G)
    # in most groups several orders fall on one unit: on plants 128 and 129 rule r + 1 then reads what rule r stored
    assert sum(len({(o[0], o[2]["unit"]) for o in g}) <= len(g) - 3 for g in G) >= (3 * len(G)) // 4
    spec = cos.value_spec()
    dec = controls.Decoder(spec, cos.SWEEP_N)
    for g in (G[0], G[-1], [TABLE[0]]):
        rules = _lib.control_orders_request(cos.group_rules(g))
        assert [D["axis"] for D in rules] == list(range(len(g)))
        orders = controls.Orders(rules, spec, cos.SWEEP_N)
        x, want = cos.sweep_inputs(len(g))
        out = dec.step(x, {})
        fire = orders.step(out["held"], out["latch"], out["restart"])
        assert np.array_equal(fire, want)
        p = np.arange(cos.SWEEP_N)
        assert not fire[:, 64:128].any() and fire[:, 128:].all()
        assert (fire[:, :64].sum(axis=0) == (p[:64] % 8 < len(g))).all()
        assert np.array_equal(orders.since, np.where(want, 1, cos.NEVER))
        for (name, kw), row in zip(orders.calls(fire), want):
            assert np.array_equal(kw["mask"] != 0, row), name


def test_the_pokes_name_fields_of_the_schema_once_each():
    rows = cos.sweep_pokes()
    keys = [(name, instance, k) for name, instance, k, _v in rows]
    assert len(set(keys)) == len(keys)
    from nuclear_sim_amd.env import SCHEMA
    for name, instance, k, v in rows:
        kind, _slot = SCHEMA.slot(name, instance, k)
        assert (kind == "i32") == (v.dtype == np.int32) and v.shape == (cos.SWEEP_N,), name
    units = {}
    for name, instance, k, _v in rows:
        units.setdefault(name.split(".")[0], set()).add((instance, k) if name.startswith(("turb.bearing", "tstg.", "cond.ej_")) else instance)
    assert units["pump"] == {0, 1, 2, 3} and {u for u in units["sg"]} == {0, 1, 2}
    assert {k for u in units["tstg"] for k in [u[1]]} == set(range(14))


@pytest.mark.parametrize("mode, families", [("primary_sg", {"pump", "steam_generator", "steam_generator_system"}), ("primary", {"pump"})])
def test_the_other_modes_accept_their_families_of_the_table_only(mode, families):
    for component, name, opt in TABLE:
        why = cos.accepted(component, name, opt, mode=mode)
        assert (why is None) == (component in families), (component, name, why)
        if why is not None:
            assert "the %r mode does not step the" % mode in why
