"""CPU: the episode records (npb_set_episode_records / npb_episode_records_check) are declared by include/npb.h, exported by libnpb.so
and bound; the binding lays the descriptor out as a C compiler does (a small compiled probe prints sizeof and every offsetof); the
library's own check, which needs no handle and reads no memory, accepts a valid descriptor and names every refusal; the env's keyword
checks come before any device work.  No compute calls.

The header keeps NPB_VERSION where the suites of the two entry-point groups before this one pin it (== 154): the new entry points are
detected by name, as npb_set_episode_streams is."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nuclear_sim_amd", "libnpb.so")
ENTRY_POINTS = ("npb_set_episode_records", "npb_episode_records_check")
FIELDS = ("capacity", "clear_summary", "plant", "episode", "start", "length", "flags", "trip_flags", "step", "ret", "end_time", "final_obs",
          "first_created", "first_completed", "n_created", "n_completed", "cursor")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nuclear_sim_amd", "csrc"), "-s"])
    from nuclear_sim_amd import _lib
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "npb.h")).read()


def test_header_declares_the_entry_points_the_descriptor_and_the_abandoned_rule():
    text = _header()
    declared = set(re.findall(r"NPB_API[^;]*?\b(npb_\w+)\s*\(", text))
    for s in ENTRY_POINTS:
        assert s in declared, s
    body = re.search(r"typedef struct npb_episode_records_desc_t \{(.*?)\} npb_episode_records_desc_t;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip().split(" ", 1)[-1])]
    assert tuple(names) == FIELDS
    assert "ABANDONS" in text and "writes NO record" in text
    assert int(re.search(r"#define NPB_VERSION (\d+)", text).group(1)) >= 154


def test_library_exports_and_binding_declares_them(L):
    raw = ctypes.CDLL(LIB)
    for s in ENTRY_POINTS:
        assert hasattr(raw, s), "libnpb.so does not export %s" % s
        assert getattr(L, s).argtypes is not None, s
    assert L.npb_version() == int(re.search(r"#define NPB_VERSION (\d+)", _header()).group(1))
    assert L.npb_set_episode_records(None, None) == -1


def test_the_binding_lays_the_descriptor_out_as_the_compiler_does(tmp_path):
    from nuclear_sim_amd import _lib
    assert tuple(f[0] for f in _lib.NpbEpisodeRecordsDesc._fields_) == FIELDS
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "npb.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(npb_episode_records_desc_t));\n'
                   + "".join('  printf("%%zu\\n", offsetof(npb_episode_records_desc_t, %s));\n' % f for f in FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    D = _lib.NpbEpisodeRecordsDesc
    assert got[0] == ctypes.sizeof(D) == 8 + 15 * 8
    assert got[1:] == [getattr(D, f).offset for f in FIELDS]
    assert [np_type().itemsize for _, np_type in _lib.EPISODE_RECORD_COLUMNS] == [4, 4, 4, 4, 4, 4, 4, 8, 8]
    assert tuple(name for name, _ in _lib.EPISODE_RECORD_COLUMNS) == FIELDS[2:11]


def _desc(summary=False, **over):
    """a descriptor whose columns are made-up, aligned addresses: the check reads no memory"""
    from nuclear_sim_amd import _lib
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


def test_the_check_accepts_a_valid_descriptor_and_names_every_refusal(L):
    def why(d, autoreset=1, keys=0):
        m = L.npb_episode_records_check(ctypes.byref(d), autoreset, keys)
        return None if m is None else m.decode()
    assert L.npb_episode_records_check(None, 0, 0) is None      # NULL turns the records off
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
