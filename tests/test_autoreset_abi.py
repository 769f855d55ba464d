"""CPU: the episode entry points (snapshot, restore, autoreset, episode buffers) are declared by include/npb.h and exported by
libnpb.so, and the Python surface refuses a time limit without autoreset before it looks for a device.  No compute calls."""
import pytest

import abi_support as abi

EPISODE_ENTRY_POINTS = ("npb_snapshot", "npb_restore", "npb_set_autoreset", "npb_set_episode_buffers")


def test_header_declares_the_episode_entry_points():
    assert set(EPISODE_ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_VERSION") >= 143


def test_library_exports_the_episode_entry_points():
    abi.check_exported(EPISODE_ENTRY_POINTS)
    assert abi.library().npb_version() >= 143


def test_binding_declares_the_episode_entry_points():
    abi.check_bound(EPISODE_ENTRY_POINTS)


def test_null_handle_is_refused():
    abi.check_null_refused([("npb_snapshot", None, None), ("npb_restore", None, None, None), ("npb_set_autoreset", None, 1, 0),
                            ("npb_set_episode_buffers", None, None, None, None, None)])


def test_time_limit_without_autoreset_is_refused():
    from nuclear_sim_amd.env import BatchedPlantEnv
    abi.library()
    with pytest.raises(ValueError):
        BatchedPlantEnv(4, max_episode_steps=7)
    with pytest.raises(ValueError):
        BatchedPlantEnv.action_test("oil_top_off", seeds=range(4), max_episode_steps=7)
