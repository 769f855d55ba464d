"""CPU: the entry points that carry the diagnostics rows through restores, resets and checkpoints, and the episode index, are
declared by include/npb.h, exported by libnpb.so and bound; the header's one table of carried rows (NPB_DIAG_CARRIED) is what the
library reports and what the binding's DIAG_CARRIED_ROWS holds.  No compute calls."""
import math
import os
import re

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

ENTRY_POINTS = ("npb_diag_num_carried", "npb_diag_carried_row", "npb_diag_carried_fresh", "npb_carry_diagnostics",
                "npb_get_diagnostics_state", "npb_set_diagnostics_state", "npb_set_episode_index_buffer")


def test_header_declares_the_entry_points():
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_VERSION") >= 151


def test_library_exports_the_entry_points():
    abi.check_exported(ENTRY_POINTS)
    assert abi.library().npb_version() >= 151


def test_binding_declares_the_entry_points():
    abi.check_bound(ENTRY_POINTS[1:])


def test_the_header_states_the_carried_rows_once_and_library_and_binding_agree():
    """the X-macro of include/npb.h, evaluated here from the header's own NPB_DIAG_* enumerators, against npb_diag_carried_row /
    npb_diag_carried_fresh and against _lib.DIAG_CARRIED_ROWS, in order"""
    text = abi.header_text()
    enum = {k: int(v) for k, v in re.findall(r"\b(NPB_DIAG_\w+) = (\d+)", text)}
    assert text.count("#define NPB_DIAG_CARRIED(X)") == 1
    body = re.search(r"#define NPB_DIAG_CARRIED\(X\)(.*?)\nenum \{ NPB_DIAG_NUM_CARRIED = (\d+) \};", text, flags=re.S)
    entries = re.findall(r"X\((NPB_DIAG_\w+)(?: \+ (\d+))?, ([0-9.]+)\)", body.group(1))
    table = [(enum[name] + int(off or 0), float(fresh)) for name, off, fresh in entries]
    assert len(table) == int(body.group(2)) == 13
    L = abi.library()
    assert L.npb_diag_num_carried() == 13
    assert [(L.npb_diag_carried_row(k), L.npb_diag_carried_fresh(k)) for k in range(13)] == table
    assert list(_lib.DIAG_CARRIED_ROWS.items()) == table
    assert sorted(r for r, _ in table) == [124, 125, 126, 127, 128, 133, 141, 142, 143, 164, 165, 166, 167]
    assert L.npb_diag_carried_row(-1) == -1 and L.npb_diag_carried_row(13) == -1 and math.isnan(L.npb_diag_carried_fresh(13))


def test_null_handle_is_refused():
    abi.check_null_refused([("npb_carry_diagnostics", None, 1), ("npb_get_diagnostics_state", None, None, None),
                            ("npb_set_diagnostics_state", None, None, None), ("npb_set_episode_index_buffer", None, None)])


def test_diagnostics_flag_is_refused_outside_the_full_mode_before_any_device_work():
    from nuclear_sim_amd.env import BatchedPlantEnv
    abi.library()
    with pytest.raises(ValueError, match="diagnostics"):
        BatchedPlantEnv(4, mode="primary", diagnostics=True)


def test_reference_reset_fixture_covers_the_table():
    """tests/golden/diag_carry/reference_reset.json (tools/make_diag_reset_golden.py): one entry per carried row, in table order, each
    either kept or reset to a value"""
    import json
    rows = json.load(open(os.path.join(abi.ROOT, "tests", "golden", "diag_carry", "reference_reset.json")))["rows"]
    assert [r["row"] for r in rows] == list(_lib.DIAG_CARRIED_ROWS)
    for r in rows:
        assert r["before_reset"] != r["fresh"], r       # the quantity had been moved, so the reset's effect on it was visible
        assert (r["rule"] == "kept" and r["reset_to"] is None and r["after_reset"] == r["before_reset"]) or \
               (r["rule"] == "reset" and r["reset_to"] == r["after_reset"]), r
