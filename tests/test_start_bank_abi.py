"""CPU: the start-bank entry points (npb_set_start_bank, npb_set_start_slots, npb_restore_bank, npb_set_episode_start_buffer) are
declared by include/npb.h, exported by libnpb.so and declared by the binding, and refuse a NULL handle.  No compute calls."""
import abi_support as abi

BANK_ENTRY_POINTS = ("npb_set_start_bank", "npb_set_start_slots", "npb_restore_bank", "npb_set_episode_start_buffer")


def test_header_declares_the_bank_entry_points():
    assert set(BANK_ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_VERSION") >= 144


def test_library_exports_the_bank_entry_points():
    abi.check_exported(BANK_ENTRY_POINTS)
    assert abi.library().npb_version() >= 144


def test_binding_declares_the_bank_entry_points():
    abi.check_bound(BANK_ENTRY_POINTS)


def test_null_handle_is_refused():
    abi.check_null_refused([("npb_set_start_bank", None, None, None), ("npb_set_start_slots", None, None, None, 0),
                            ("npb_restore_bank", None, None, None), ("npb_set_episode_start_buffer", None, None)])
