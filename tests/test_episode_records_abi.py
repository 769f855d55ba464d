"""CPU: the episode records (npb_set_episode_records / npb_episode_records_check) are declared by include/npb.h, exported by libnpb.so
and bound; the binding lays the descriptor out as a C compiler does (a small compiled probe prints sizeof and every offsetof); the
library's own check, which needs no handle and reads no memory, accepts a valid descriptor and names every refusal; the env's keyword
checks come before any device work.  No compute calls.

The header keeps NPB_VERSION where the suites of the two entry-point groups before this one pin it (== 154): the new entry points are
detected by name, as npb_set_episode_streams is."""
import ctypes
import re

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

ENTRY_POINTS = ("npb_set_episode_records", "npb_episode_records_check")
FIELDS = ("capacity", "clear_summary", "plant", "episode", "start", "length", "flags", "trip_flags", "step", "ret", "end_time", "final_obs",
          "first_created", "first_completed", "n_created", "n_completed", "cursor")


def test_header_declares_the_entry_points_the_descriptor_and_the_abandoned_rule():
    text = abi.header_text()
    assert set(ENTRY_POINTS) <= set(abi.declared())
    body = re.search(r"typedef struct npb_episode_records_desc_t \{(.*?)\} npb_episode_records_desc_t;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip().split(" ", 1)[-1])]
    assert tuple(names) == FIELDS
    assert "ABANDONS" in text and "writes NO record" in text
    assert abi.define("NPB_VERSION") >= 154


def test_library_exports_and_binding_declares_them():
    abi.check_entry_points(ENTRY_POINTS, [("npb_set_episode_records", None, None)])
    assert abi.library().npb_version() == abi.define("NPB_VERSION")


def test_the_binding_lays_the_descriptor_out_as_the_compiler_does():
    D = _lib.NpbEpisodeRecordsDesc
    assert tuple(f[0] for f in D._fields_) == FIELDS
    got = abi.probe({"npb_episode_records_desc_t": D})[0]
    assert got[0] == ctypes.sizeof(D) == 8 + 15 * 8
    assert got[1:] == [getattr(D, f).offset for f in FIELDS]
    assert [np_type().itemsize for _, np_type in _lib.EPISODE_RECORD_COLUMNS] == [4, 4, 4, 4, 4, 4, 4, 8, 8]
    assert tuple(name for name, _ in _lib.EPISODE_RECORD_COLUMNS) == FIELDS[2:11]


def _desc(summary=False, **over):
    """a descriptor whose columns are made-up, aligned addresses: the check reads no memory"""
    d = _lib.NpbEpisodeRecordsDesc()
    d.capacity, d.clear_summary = 64, 0
    for k, name in enumerate(FIELDS[2:11]):
        setattr(d, name, 0x10000 + 0x1000 * k)
    d.cursor = 0x30000
    if summary:
        d.first_created, d.first_completed, d.n_created, d.n_completed = 0x40000, 0x41000, 0x42000, 0x43004
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_the_check_accepts_a_valid_descriptor_and_names_every_refusal():
    L = abi.library()

    def why(d, autoreset=1, keys=0):
        return abi.why(L.npb_episode_records_check, ctypes.byref(d), autoreset, keys)
    assert L.npb_episode_records_check(None, 0, 0) is None     # NULL turns the records off
    assert why(_desc()) is None and why(_desc(final_obs=0x50000)) is None and why(_desc(capacity=1)) is None
    assert why(_desc(summary=True), keys=3) is None and why(_desc(summary=True, clear_summary=1), keys=1) is None
    assert why(_desc(clear_summary=1), keys=2) is None          # clearing without copying
    assert "no autoreset" in why(_desc(), autoreset=0)
    assert "capacity must be >= 1" in why(_desc(capacity=0)) and "capacity must be >= 1" in why(_desc(capacity=-5))
    for member in FIELDS[2:11] + ("cursor",):
        assert "must not be NULL" in why(_desc(**{member: None})), member
    for member in FIELDS[2:9] + ("cursor",):
        assert "aligned" in why(_desc(**{member: 0x10002})), member
        assert why(_desc(**{member: 0x10004})) is None, member      # the int32 columns need four bytes only
    for member in ("ret", "end_time", "final_obs"):
        assert "aligned" in why(_desc(**{member: 0x10004})), member
    assert "aligned" in why(_desc(summary=True, first_created=0x40004), keys=1)
    assert "aligned" in why(_desc(summary=True, n_completed=0x43002), keys=1)
    for member in ("first_created", "first_completed", "n_created", "n_completed"):
        assert "only part of the four summary tables" in why(_desc(summary=True, **{member: None}), keys=1), member
        assert "only part of the four summary tables" in why(_desc(**{member: 0x40000}), keys=1), member
    assert "summary columns without a work-order summary" in why(_desc(summary=True), keys=0)
    assert "clear_summary without a work-order summary" in why(_desc(clear_summary=1), keys=0)


def test_the_env_refuses_before_any_device_work():
    from nuclear_sim_amd.env import BatchedPlantEnv
    with pytest.raises(ValueError, match="autoreset=True"):
        BatchedPlantEnv.action_test("oil_top_off", [1, 2], episode_records=True)
    with pytest.raises(ValueError, match="autoreset=True"):
        BatchedPlantEnv.action_test("oil_top_off", [1, 2], episode_records=64)
    from nuclear_sim_amd.timing import banked_trigger_times
    with pytest.raises(ValueError, match="lanes"):
        banked_trigger_times("oil_top_off", [1, 2, 3], 1.0, lanes=4)
    with pytest.raises(ValueError, match="lanes"):
        banked_trigger_times("oil_top_off", [1, 2, 3], 1.0, lanes=0)
