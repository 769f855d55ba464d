"""CPU: the entry points that carry the diagnostics rows through restores, resets and checkpoints, and the episode index, are
declared by include/npb.h, exported by libnpb.so and bound; the header's one table of carried rows (NPB_DIAG_CARRIED) is what the
library reports and what the binding's DIAG_CARRIED_ROWS holds.  No compute calls."""
import ctypes
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nuclear_sim_amd", "libnpb.so")
ENTRY_POINTS = ("npb_diag_num_carried", "npb_diag_carried_row", "npb_diag_carried_fresh", "npb_carry_diagnostics",
                "npb_get_diagnostics_state", "npb_set_diagnostics_state", "npb_set_episode_index_buffer")


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nuclear_sim_amd", "csrc"), "-s"])
    return LIB


def _header():
    return open(os.path.join(ROOT, "include", "npb.h")).read()


def test_header_declares_the_entry_points():
    text = _header()
    declared = set(re.findall(r"NPB_API[^;]*?\b(npb_\w+)\s*\(", text))
    for s in ENTRY_POINTS:
        assert s in declared, s
    assert int(re.search(r"#define NPB_VERSION (\d+)", text).group(1)) >= 151


def test_library_exports_the_entry_points(built_lib):
    lib = ctypes.CDLL(built_lib)
    for s in ENTRY_POINTS:
        assert hasattr(lib, s), "libnpb.so does not export %s" % s
    assert lib.npb_version() >= 151


def test_binding_declares_the_entry_points(built_lib):
    from nuclear_sim_amd import _lib
    L = _lib.load()
    for s in ENTRY_POINTS[1:]:
        assert getattr(L, s).argtypes is not None, s


def test_the_header_states_the_carried_rows_once_and_library_and_binding_agree(built_lib):
    """the X-macro of include/npb.h, evaluated here from the header's own NPB_DIAG_* enumerators, against npb_diag_carried_row /
    npb_diag_carried_fresh and against _lib.DIAG_CARRIED_ROWS, in order"""
    from nuclear_sim_amd import _lib
    text = _header()
    enum = {k: int(v) for k, v in re.findall(r"\b(NPB_DIAG_\w+) = (\d+)", text)}
    assert text.count("#define NPB_DIAG_CARRIED(X)") == 1
    body = re.search(r"#define NPB_DIAG_CARRIED\(X\)(.*?)\nenum \{ NPB_DIAG_NUM_CARRIED = (\d+) \};", text, flags=re.S)
    entries = re.findall(r"X\((NPB_DIAG_\w+)(?: \+ (\d+))?, ([0-9.]+)\)", body.group(1))
    table = [(enum[name] + int(off or 0), float(fresh)) for name, off, fresh in entries]
    assert len(table) == int(body.group(2)) == 13
    L = _lib.load()
    assert L.npb_diag_num_carried() == 13
    assert [(L.npb_diag_carried_row(k), L.npb_diag_carried_fresh(k)) for k in range(13)] == table
    assert list(_lib.DIAG_CARRIED_ROWS.items()) == table
    assert sorted(r for r, _ in table) == [124, 125, 126, 127, 128, 133, 141, 142, 143, 164, 165, 166, 167]
    assert L.npb_diag_carried_row(-1) == -1 and L.npb_diag_carried_row(13) == -1 and math.isnan(L.npb_diag_carried_fresh(13))


def test_null_handle_is_refused(built_lib):
    from nuclear_sim_amd import _lib
    L = _lib.load()
    assert L.npb_carry_diagnostics(None, 1) == -1
    assert L.npb_get_diagnostics_state(None, None, None) == -1
    assert L.npb_set_diagnostics_state(None, None, None) == -1
    assert L.npb_set_episode_index_buffer(None, None) == -1


def test_diagnostics_flag_is_refused_outside_the_full_mode_before_any_device_work(built_lib):
    from nuclear_sim_amd.env import BatchedPlantEnv
    with pytest.raises(ValueError, match="diagnostics"):
        BatchedPlantEnv(4, mode="primary", diagnostics=True)


def test_reference_reset_fixture_covers_the_table(built_lib):
    """tests/golden/diag_carry/reference_reset.json (tools/make_diag_reset_golden.py): one entry per carried row, in table order, each
    either kept or reset to a value"""
    import json
    from nuclear_sim_amd import _lib
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "diag_carry", "reference_reset.json")))["rows"]
    assert [r["row"] for r in rows] == list(_lib.DIAG_CARRIED_ROWS)
    for r in rows:
        assert r["before_reset"] != r["fresh"], r       # the quantity had been moved, so the reset's effect on it was visible
        assert (r["rule"] == "kept" and r["reset_to"] is None and r["after_reset"] == r["before_reset"]) or \
               (r["rule"] == "reset" and r["reset_to"] == r["after_reset"]), r
