"""CPU: the episode entry points (snapshot, restore, autoreset, episode buffers) are declared by include/npb.h and exported by
libnpb.so, and the Python surface refuses a time limit without autoreset before it looks for a device.  No compute calls."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nuclear_sim_amd", "libnpb.so")
EPISODE_ENTRY_POINTS = ("npb_snapshot", "npb_restore", "npb_set_autoreset", "npb_set_episode_buffers")


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nuclear_sim_amd", "csrc"), "-s"])
    return LIB


def test_header_declares_the_episode_entry_points():
    text = open(os.path.join(ROOT, "include", "npb.h")).read()
    declared = set(re.findall(r"NPB_API[^;]*?\b(npb_\w+)\s*\(", text))
    for s in EPISODE_ENTRY_POINTS:
        assert s in declared, s
    assert int(re.search(r"#define NPB_VERSION (\d+)", text).group(1)) >= 143


def test_library_exports_the_episode_entry_points(built_lib):
    lib = ctypes.CDLL(built_lib)
    for s in EPISODE_ENTRY_POINTS:
        assert hasattr(lib, s), "libnpb.so does not export %s" % s
    assert lib.npb_version() >= 143


def test_binding_declares_the_episode_entry_points(built_lib):
    from nuclear_sim_amd import _lib
    L = _lib.load()
    for s in EPISODE_ENTRY_POINTS:
        assert getattr(L, s).argtypes is not None, s


def test_null_handle_is_refused(built_lib):
    from nuclear_sim_amd import _lib
    L = _lib.load()
    assert L.npb_snapshot(None, None) == -1
    assert L.npb_restore(None, None, None) == -1
    assert L.npb_set_autoreset(None, 1, 0) == -1
    assert L.npb_set_episode_buffers(None, None, None, None, None) == -1


def test_time_limit_without_autoreset_is_refused(built_lib):
    from nuclear_sim_amd.env import BatchedPlantEnv
    with pytest.raises(ValueError):
        BatchedPlantEnv(4, max_episode_steps=7)
    with pytest.raises(ValueError):
        BatchedPlantEnv.action_test("oil_top_off", seeds=range(4), max_episode_steps=7)
