"""CPU: the start-bank entry points (npb_set_start_bank, npb_set_start_slots, npb_restore_bank, npb_set_episode_start_buffer) are
declared by include/npb.h, exported by libnpb.so and declared by the binding, and refuse a NULL handle.  No compute calls."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nuclear_sim_amd", "libnpb.so")
BANK_ENTRY_POINTS = ("npb_set_start_bank", "npb_set_start_slots", "npb_restore_bank", "npb_set_episode_start_buffer")


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nuclear_sim_amd", "csrc"), "-s"])
    return LIB


def test_header_declares_the_bank_entry_points():
    text = open(os.path.join(ROOT, "include", "npb.h")).read()
    declared = set(re.findall(r"NPB_API[^;]*?\b(npb_\w+)\s*\(", text))
    for s in BANK_ENTRY_POINTS:
        assert s in declared, s
    assert int(re.search(r"#define NPB_VERSION (\d+)", text).group(1)) >= 144


def test_library_exports_the_bank_entry_points(built_lib):
    lib = ctypes.CDLL(built_lib)
    for s in BANK_ENTRY_POINTS:
        assert hasattr(lib, s), "libnpb.so does not export %s" % s
    assert lib.npb_version() >= 144


def test_binding_declares_the_bank_entry_points(built_lib):
    from nuclear_sim_amd import _lib
    L = _lib.load()
    for s in BANK_ENTRY_POINTS:
        assert getattr(L, s).argtypes is not None, s


def test_null_handle_is_refused(built_lib):
    from nuclear_sim_amd import _lib
    L = _lib.load()
    assert L.npb_set_start_bank(None, None, None) == -1
    assert L.npb_set_start_slots(None, None, None, 0) == -1
    assert L.npb_restore_bank(None, None, None) == -1
    assert L.npb_set_episode_start_buffer(None, None) == -1
