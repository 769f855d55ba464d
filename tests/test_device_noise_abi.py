"""CPU: the device noise entry points (npb_noise_seed, npb_noise_fill, npb_noise_get_state, npb_noise_set_state) are declared by
include/npb.h, exported by libnpb.so and declared by the binding, and refuse a NULL handle; the binding's noise_generator keyword
refuses an unknown generator.  No compute calls."""
import pytest

import abi_support as abi

NOISE_ENTRY_POINTS = ("npb_noise_seed", "npb_noise_fill", "npb_noise_get_state", "npb_noise_set_state")


def test_header_declares_the_noise_entry_points():
    assert set(NOISE_ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_VERSION") >= 145


def test_library_exports_the_noise_entry_points():
    abi.check_exported(NOISE_ENTRY_POINTS)
    assert abi.library().npb_version() >= 145


def test_binding_declares_the_noise_entry_points():
    abi.check_bound(NOISE_ENTRY_POINTS)


def test_null_handle_is_refused():
    abi.check_null_refused([("npb_noise_seed", None, None, None), ("npb_noise_fill", None, 1, None, None),
                            ("npb_noise_get_state", None, None, None, None, None, None),
                            ("npb_noise_set_state", None, None, None, None, None, None)])


def test_unknown_noise_generator_is_refused():
    from nuclear_sim_amd.env import BatchedPlantEnv
    abi.library()
    with pytest.raises(ValueError):
        BatchedPlantEnv(4, noise_enabled=True, noise_generator="gpu")
