"""CPU: the sampler of a state log with a watch list (npb_sampler_create / npb_sampler_sample / npb_sampler_destroy) is declared by
include/npb.h, exported by libnpb.so and bound; the watch list's validator and the builder of the sample request are pure host
functions and are checked here without a device.  No compute calls."""
import ctypes
import re

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

ENTRY_POINTS = ("npb_sampler_create", "npb_sampler_sample", "npb_sampler_destroy")


def test_header_declares_the_entry_points():
    text, declared = abi.header_text(), set(abi.declared())
    for s in ENTRY_POINTS:
        assert s in declared, s
    assert abi.define("NPB_VERSION") >= 153


def test_library_exports_the_entry_points():
    abi.check_exported(ENTRY_POINTS)
    assert abi.library().npb_version() >= 153


def test_binding_declares_the_entry_points_and_the_request_as_the_header_lays_it_out():
    L = abi.library()
    for s in ENTRY_POINTS:
        assert getattr(L, s).argtypes is not None, s
    text = abi.header_text()
    types = dict((name, int(v)) for name, v in re.findall(r"\b(NPB_SAMPLE_\w+) = (\d+)", text))
    assert {k: types["NPB_SAMPLE_" + k.upper()] for k in _lib.SAMPLE_TYPES} == _lib.SAMPLE_TYPES
    # the two structs: field names in the header's order
    src = re.search(r"typedef struct \{([^}]*)\} npb_sample_source_t;", text).group(1)
    assert re.findall(r"(\w+)\s*[,;]", src) == [f[0] for f in _lib.NpbSampleSource._fields_]
    desc = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} npb_sampler_desc_t;", text, flags=re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+)\s*;", desc) == [f[0] for f in _lib.NpbSamplerDesc._fields_]
    assert ctypes.sizeof(_lib.NpbSampleSource) == 32


def test_null_handle_is_refused():
    L = abi.library()
    sampler = ctypes.c_int(7)
    desc = _lib.NpbSamplerDesc()
    assert L.npb_sampler_create(None, ctypes.byref(desc), ctypes.byref(sampler)) == -1
    assert b"npb_sampler_create: NULL handle" in L.npb_last_error(None)
    assert L.npb_sampler_sample(None, 0, None, None) == -1
    assert b"npb_sampler_sample: NULL handle" in L.npb_last_error(None)
    assert L.npb_sampler_destroy(None, 0) == -1
    assert b"npb_sampler_destroy: NULL handle" in L.npb_last_error(None)


@pytest.mark.parametrize("ids, named", [([], "empty"), ([-1], "-1"), ([10], "10"), ([3, 3], "3"), ([1.5], "1.5")])
def test_the_validator_refuses_a_bad_watch_list_by_a_message_naming_the_id(ids, named):
    from nuclear_sim_amd.statelog import validate_watch_list
    with pytest.raises(ValueError, match=re.escape(named)):
        validate_watch_list(ids, 10)


def test_the_validator_returns_the_ids_sorted():
    import numpy as np
    from nuclear_sim_amd.statelog import validate_watch_list
    assert validate_watch_list([199, 0, 63, 64, 65, 128, 7], 200) == [0, 7, 63, 64, 65, 128, 199]
    assert validate_watch_list(np.array([5, 2, 9]), 10) == [2, 5, 9]
    assert validate_watch_list(range(4), 4) == [0, 1, 2, 3]
    import torch
    assert validate_watch_list(torch.tensor([4, 1]), 5) == [1, 4]
    with pytest.raises(ValueError, match="2.5"):
        validate_watch_list(np.array([2.5, 1.0]), 5)
    assert all(type(p) is int for p in validate_watch_list(np.array([5, 2], dtype=np.int32), 10))
    with pytest.raises(ValueError, match="True"):
        validate_watch_list([True], 10)


def _reference_request(**kw):
    from nuclear_sim_amd.statelog import log_columns, sample_request
    cols = log_columns(None)
    return cols, sample_request(cols, **kw)


def test_the_request_of_the_reference_layout_lists_every_member_exactly_once():
    from nuclear_sim_amd.env import SECONDARY_RESULT_MEMBERS
    from nuclear_sim_amd.schema import SCHEMA
    cols, req = _reference_request(result=True, diagnostics=True, outputs=True, episodic=True, diag_pitch=256)
    keys = [(kind, slot) for kind, slot, _label in req["members"]]
    assert len(keys) == len(set(keys))
    # the logged columns first and in their order: rows 0 .. nf - 1 are what array() returns
    assert keys[:len(cols)] == [(c[0], c[1]) for c in cols]
    # every member the secondary result is formed from has its row, the logged ones without a second one
    assert set(req["secondary"]) == set(SECONDARY_RESULT_MEMBERS)
    logged = {(c[0], c[1]): f for f, c in enumerate(cols)}
    extra = 0
    for name in SECONDARY_RESULT_MEMBERS:
        key = SCHEMA.slot(name)
        assert keys[req["secondary"][name]] == key
        if key in logged:
            assert req["secondary"][name] == logged[key]
        else:
            extra += 1
    assert len(keys) == len(cols) + extra
    assert set(keys) == set(logged) | {SCHEMA.slot(name) for name in SECONDARY_RESULT_MEMBERS}


def test_the_side_sources_come_in_the_documented_order_with_the_documented_strides():
    cols, req = _reference_request(result=True, diagnostics=True, outputs=True, episodic=True, diag_pitch=256)
    sides = req["sides"]
    assert [(s["name"], s["type"], s["rows"], s["row_stride"], s["plant_stride"]) for s in sides] == [
        ("info", "f64", _lib.INFO_DIM, 1, _lib.INFO_DIM),            # [n][NPB_INFO_DIM]
        ("diagnostics", "f64", _lib.DIAG_DIM, 256, 1),               # [NPB_DIAG_DIM][pitch]
        ("done", "u8", 1, 0, 1),
        ("truncated", "u8", 1, 0, 1), ("episode_index", "i32", 1, 0, 1), ("episode_length", "i32", 1, 0, 1)]
    row = len(req["members"])
    for s in sides:      # behind the members, one after the other
        assert s["row"] == row
        row += s["rows"]
    assert req["rows"] == row == len(req["members"]) + 17 + 170 + 4


def test_the_request_follows_the_flags():
    from nuclear_sim_amd.statelog import log_columns, sample_request
    cols = log_columns(["pump.oil_level"])
    req = sample_request(cols)
    assert req["sides"] == [] and req["secondary"] == {} and req["rows"] == len(cols) == len(req["members"])
    req = sample_request(cols, outputs=True, episodic=True)
    assert [s["name"] for s in req["sides"]] == ["done", "truncated", "episode_index", "episode_length"]
    _cols, req = _reference_request(result=True, outputs=True)
    assert [s["name"] for s in req["sides"]] == ["info", "done"]
