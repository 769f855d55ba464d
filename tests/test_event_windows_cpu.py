"""CPU: the event windows (npb_set_event_windows, npb_event_windows_check, npb_event_windows_clear, npb_event_windows_bytes) are declared
by include/npb.h, exported by libnpb.so and bound, the binding laying the descriptor and the trigger out as a C compiler does; the
library's own check, which needs no handle and reads no device memory, accepts a good descriptor and names every refusal; the request
builder of the binding refuses unknown triggers and a work_order trigger without a summary before any device work; and eventwin.record,
the numpy statement of what the device captures, on hand-made series.  No compute calls."""
import ctypes

import numpy as np
import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

ENTRY_POINTS = ("npb_set_event_windows", "npb_event_windows_check", "npb_event_windows_clear", "npb_event_windows_bytes")
WORDS = ("plant", "episode", "trigger", "step", "n_pre", "n_post", "flags", "retriggers", "fired")
RECORD = WORDS + ("time", "times", "values", "cursor")
DESC_FIELDS = ("n_fields", "kinds", "slots", "n_sources", "sources", "n_triggers", "triggers", "pre", "post", "capacity") + RECORD
TRIGGER_FIELDS = ("from_source", "kind", "slot", "source", "mode", "mask", "direction", "limit")
BITS, INCREASE, BEYOND = 0, 1, 2


@pytest.fixture(scope="module")
def L():
    return abi.library()


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_the_four_entry_points_and_keeps_the_version():
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_VERSION") == 154
    assert abi.define("NPB_EVENT_WINDOW_COLS_MAX") == 16
    assert abi.define("NPB_EVENT_WINDOW_TRIGGERS_MAX") == 8


def test_library_exports_and_binding_declares_them(L):
    from nuclear_sim_amd import eventwin
    abi.check_entry_points(ENTRY_POINTS, [("npb_set_event_windows", None, None), ("npb_event_windows_clear", None, None, None)])
    assert L.npb_version() == 154
    assert L.npb_event_windows_bytes(None, 70) == 0
    assert (_lib.EVENT_WINDOW_COLS_MAX, _lib.EVENT_WINDOW_TRIGGERS_MAX, _lib.EVENT_WINDOW_ROWS_MAX) == \
        (eventwin.MAX_COLUMNS, eventwin.MAX_TRIGGERS, eventwin.MAX_ROWS) == (16, 8, 1024)
    assert _lib.EVENT_WINDOW_WORDS == eventwin.WORD_COLUMNS and _lib.TRIGGER_MODES == {"bits_rise": BITS, "increase": INCREASE, "beyond": BEYOND}


def test_the_binding_lays_the_descriptor_and_the_trigger_out_as_the_compiler_does():
    A, B = _lib.NpbEventWindowsDesc, _lib.NpbEventTrigger
    assert tuple(f[0] for f in A._fields_) == DESC_FIELDS
    assert tuple(f[0] for f in B._fields_) == TRIGGER_FIELDS
    triggers = ["((npb_event_trigger_t){0, 1, 2, {0}, %s})" % m for m in ("NPB_TRIGGER_BITS_RISE(5)", "NPB_TRIGGER_INCREASE", "NPB_TRIGGER_BEYOND(-1, 2.5)")]
    got, values = abi.probe({"npb_event_windows_desc_t": A, "npb_event_trigger_t": B},
                            [m % t for t in triggers for m in ("%s.mode", "%s.mask", "%s.direction", "(int)(%s.limit * 2)")], std="c99")
    k = 1 + len(DESC_FIELDS)
    assert got[0] == ctypes.sizeof(A) and got[1:k] == [getattr(A, f).offset for f in DESC_FIELDS]
    assert got[k] == ctypes.sizeof(B) and got[k + 1:] == [getattr(B, f).offset for f in TRIGGER_FIELDS]
    assert values == [BITS, 5, 0, 0, INCREASE, 0, 0, 0, BEYOND, 0, -1, 5]      # the three initialiser macros


def _good(n_fields=2, n_sources=2, pre=3, post=2, capacity=64):
    """a descriptor the check accepts (it reads no device memory: the addresses only have to be aligned), and what keeps it alive.
    Triggers: rising bits of an I32 source, an increase of an int32 member, a limit on a carried member, a limit on an F64 source"""
    from nuclear_sim_amd.schema import SCHEMA
    d = _lib.NpbEventWindowsDesc()
    members = [SCHEMA.slot("pump.oil_level", 0), SCHEMA.slot("maint.maintenance_actions_performed")][:n_fields]
    members += [SCHEMA.slot("pump.oil_level", 1)] * (n_fields - len(members))
    kinds = (ctypes.c_int * max(n_fields, 1))(*[0 if k == "f64" else 1 for k, _ in members])
    slots = (ctypes.c_int * max(n_fields, 1))(*[s for _, s in members])
    side = (_lib.NpbSampleSource * max(n_sources, 1))()
    for k in range(n_sources):
        side[k].base, side[k].type, side[k].rows, side[k].row_stride, side[k].plant_stride = 0x10000 + 64 * k, 0, 1, 0, 17
    trig = (_lib.NpbEventTrigger * 4)()
    trig[0].from_source = 1
    trig[0].source.base, trig[0].source.type, trig[0].source.rows, trig[0].source.plant_stride = 0x30000, 2, 1, 1
    trig[0].mode, trig[0].mask = BITS, 0xFF
    trig[1].kind, trig[1].slot, trig[1].mode = 1, SCHEMA.slot("maint.maintenance_actions_performed")[1], INCREASE
    trig[2].kind, trig[2].slot, trig[2].mode, trig[2].direction, trig[2].limit = 0, SCHEMA.slot("pump.oil_level", 0)[1], BEYOND, -1, 30.0
    trig[3].from_source = 1
    trig[3].source.base, trig[3].source.type, trig[3].source.rows, trig[3].source.plant_stride = 0x40000, 0, 1, 17
    trig[3].mode, trig[3].direction, trig[3].limit = BEYOND, 1, 900.0
    d.n_fields, d.kinds, d.slots, d.n_sources, d.sources, d.n_triggers, d.triggers = n_fields, kinds, slots, n_sources, side, 4, trig
    d.pre, d.post, d.capacity = pre, post, capacity
    for j, name in enumerate(RECORD):
        setattr(d, name, 0x200000 + 0x10000 * j)
    return d, (kinds, slots, side, trig)


def _why(L, d, n=70):
    r = L.npb_event_windows_check(ctypes.byref(d), n, 0)
    return None if r is None else r.decode()


def test_check_accepts_a_good_descriptor_and_bytes_counts_the_ring(L):
    d, keep = _good()
    assert _why(L, d) is None
    assert L.npb_event_windows_check(None, 70, 1) is None            # NULL = off
    assert L.npb_event_windows_check(ctypes.byref(d), 70, 1) is None
    # the ring [H][n_cols + 1][n], prev [n_triggers][n], nine words per plant (one of them a double), and the two small tables
    H, n = 6, 70
    fixed = L.npb_event_windows_bytes(ctypes.byref(d), n) - (H * 5 + 4 + 1) * n * 8 - 8 * n * 4
    assert 0 < fixed < 4096
    d2, keep2 = _good(pre=8, post=8)
    assert L.npb_event_windows_bytes(ctypes.byref(d2), 2 * n) - fixed == (17 * 5 + 4 + 1) * 2 * n * 8 + 8 * 2 * n * 4
    for kw in (dict(n_fields=16, n_sources=0), dict(n_fields=0, n_sources=1), dict(pre=0, post=0), dict(pre=1000, post=23), dict(capacity=1)):
        d, keep = _good(**kw)
        assert _why(L, d) is None, kw
    d, keep = _good()
    d.n_triggers = 1
    assert _why(L, d) is None
    keep[3][0].source.type = 3                                        # rising bits of a U8 source (the done column)
    assert _why(L, d) is None


def test_check_names_every_refusal(L):
    def refused(change, word, **kw):
        d, keep = _good(**kw)
        change(d, keep)
        why = _why(L, d)
        assert why is not None and why.startswith("npb_set_event_windows:") and word in why, (word, why)
        assert L.npb_event_windows_bytes(ctypes.byref(d), 70) == 0      # nothing to allocate for a descriptor that is refused

    refused(lambda d, k: None, "column count", n_fields=0, n_sources=0)
    refused(lambda d, k: None, "column count", n_fields=16, n_sources=1)
    refused(lambda d, k: setattr(d, "n_fields", -1), "column count")
    refused(lambda d, k: setattr(d, "n_triggers", 0), "trigger count")
    refused(lambda d, k: setattr(d, "n_triggers", 9), "trigger count")
    refused(lambda d, k: setattr(d, "triggers", None), "trigger count")
    refused(lambda d, k: None, "window shape", pre=-1)
    refused(lambda d, k: None, "window shape", post=-1)
    refused(lambda d, k: None, "window shape", pre=1000, post=24)
    refused(lambda d, k: None, "capacity must be >= 1", capacity=0)
    refused(lambda d, k: k[0].__setitem__(0, 2), "bad field kind or slot")
    refused(lambda d, k: k[1].__setitem__(1, 1 << 20), "bad field kind or slot")
    refused(lambda d, k: k[1].__setitem__(0, -1), "bad field kind or slot")
    refused(lambda d, k: setattr(k[3][1], "slot", 1 << 20), "bad field kind or slot")      # a trigger's member
    refused(lambda d, k: setattr(k[3][2], "kind", 7), "bad field kind or slot")
    refused(lambda d, k: setattr(k[2][1], "base", None), "NULL base")
    refused(lambda d, k: setattr(k[2][0], "type", 4), "unknown element type")
    refused(lambda d, k: setattr(k[2][0], "type", -1), "unknown element type")
    refused(lambda d, k: setattr(k[2][0], "rows", 2), "rows == 1")
    refused(lambda d, k: setattr(k[2][0], "rows", 0), "rows == 1")
    refused(lambda d, k: setattr(k[3][0].source, "base", None), "NULL base")             # a trigger's source
    refused(lambda d, k: setattr(k[3][3].source, "type", 9), "unknown element type")
    refused(lambda d, k: setattr(k[3][0].source, "rows", 3), "rows == 1")
    refused(lambda d, k: setattr(k[3][0].source, "type", 0), "real-valued")              # BITS_RISE on an F64 source
    refused(lambda d, k: setattr(k[3][0].source, "type", 1), "real-valued")              # ... an F32 source
    refused(lambda d, k: setattr(k[3][2], "mode", BITS), "real-valued")                  # ... a carried fp64 member
    refused(lambda d, k: setattr(k[3][0], "mask", 0), "mask 0")
    refused(lambda d, k: setattr(k[3][1], "mode", 3), "unknown trigger mode")
    refused(lambda d, k: setattr(k[3][2], "limit", float("nan")), "NaN limit")
    refused(lambda d, k: setattr(k[3][2], "direction", 0), "direction outside")
    refused(lambda d, k: setattr(k[3][3], "direction", 2), "direction outside")
    for name in RECORD:
        refused(lambda d, k, name=name: setattr(d, name, None), "NULL record column or cursor")
    for name in WORDS + ("cursor",):
        refused(lambda d, k, name=name: setattr(d, name, getattr(d, name) + 2), "misaligned record column")
    for name in ("time", "times", "values"):
        refused(lambda d, k, name=name: setattr(d, name, getattr(d, name) + 4), "misaligned record column")


# ---------------------------------------------------------------------------------------------------------------- the request builder
def test_request_builder_maps_the_triggers():
    from nuclear_sim_amd.env import INFO_COLUMNS
    from nuclear_sim_amd.schema import SCHEMA
    req = _lib.event_windows_request(["reward", ("pump.oil_level", 1), ("obs", 3)],
                                     [("trip", 0x30), ("done",), ("work_order", 1), ("completed", 0), ("maintenance",),
                                      (("pump.oil_level", 0), "<", 30.0), (("info", "electrical_power"), ">", 900.0), ("reward", "<", -1.0)],
                                     3, 2, summary_keys=2)
    assert req["members"] == [(0, SCHEMA.slot("pump.oil_level", 1)[1])] and req["sides"] == [("reward", 0, 1), ("obs", 3, 22)]
    assert req["order"] == [1, 0, 2] and (req["pre"], req["post"]) == (3, 2)
    t = req["triggers"]
    assert (t[0]["side"], t[0]["mode"], t[0]["mask"]) == (("flags", 0, 1, "i32"), "bits_rise", 0x30)
    assert (t[1]["side"], t[1]["mode"], t[1]["mask"]) == (("done", 0, 1, "u8"), "bits_rise", 1)
    assert (t[2]["side"], t[2]["mode"]) == (("n_created", 1, 1, "i32"), "increase") and (t[3]["side"], t[3]["mode"]) == (("n_completed", 0, 1, "i32"), "increase")
    assert t[4]["member"] == (1, SCHEMA.slot("maint.maintenance_actions_performed")[1]) and t[4]["mode"] == "increase" and t[4]["side"] is None
    assert (t[5]["member"], t[5]["mode"], t[5]["direction"], t[5]["limit"]) == ((0, SCHEMA.slot("pump.oil_level", 0)[1]), "beyond", -1, 30.0)
    assert (t[6]["side"], t[6]["direction"], t[6]["limit"]) == (("info", INFO_COLUMNS.index("electrical_power"), len(INFO_COLUMNS), "f64"), 1, 900.0)
    assert t[7]["side"] == ("reward", 0, 1, "f64")
    assert req["numpy"] == [("bits", 0x30), ("bits", 1), ("increase",), ("increase",), ("increase",), ("<", 30.0), (">", 900.0), ("<", -1.0)]


@pytest.mark.parametrize("columns, triggers, pre, post, keys, word", [
    (["reward"], [("no_such_trigger",)], 1, 1, 0, "unknown trigger"),
    (["reward"], [("trip",)], 1, 1, 0, "unknown trigger"),
    (["reward"], ["tripped"], 1, 1, 0, "unknown trigger"),
    (["reward"], [("reward", ">=", 1.0)], 1, 1, 0, "unknown trigger"),
    (["reward"], [("trip", 0)], 1, 1, 0, "mask"),
    (["reward"], [("work_order", 0)], 1, 1, 0, "enable_maintenance_summary"),
    (["reward"], [("completed", 0)], 1, 1, 0, "enable_maintenance_summary"),
    (["reward"], [("work_order", 2)], 1, 1, 2, "keys are 0 .. 1"),
    (["reward"], [("pump.no_such_member", ">", 1.0)], 1, 1, 0, "unknown column"),
    (["reward"], [(("info", "nope"), ">", 1.0)], 1, 1, 0, "unknown info column"),
    (["reward"], [("reward", ">", float("nan"))], 1, 1, 0, "NaN"),
    (["pump.no_such_member"], [("done",)], 1, 1, 0, "unknown column"),
    ([], [("done",)], 1, 1, 0, "1 to 16 columns"),
    (["reward"] * 17, [("done",)], 1, 1, 0, "1 to 16 columns"),
    (["reward"], [], 1, 1, 0, "1 to 8 triggers"),
    (["reward"], [("done",)] * 9, 1, 1, 0, "1 to 8 triggers"),
    (["reward"], [("done",)], -1, 1, 0, "pre >= 0"),
    (["reward"], [("done",)], 1000, 24, 0, "<= 1024"),
])
def test_request_builder_refuses(columns, triggers, pre, post, keys, word):
    with pytest.raises(ValueError) as e:
        _lib.event_windows_request(columns, triggers, pre, post, summary_keys=keys)
    assert word in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------------- eventwin.record
def _series(trig, n_cols=2, plants=None):
    """hand-made input of `record` from trigger series [S] per plant: values 100 c + 1000 p + s, clock 5 (s + 1) + 10000 p"""
    tv = np.array(trig, dtype=np.float64)
    tv = tv.reshape(tv.shape[0], 1, -1) if tv.ndim <= 2 else tv
    S, _, n = tv.shape
    s, c, p = np.arange(S).reshape(S, 1, 1), np.arange(n_cols).reshape(1, n_cols, 1), np.arange(n).reshape(1, 1, n)
    return (100.0 * c + 1000.0 * p + s) * np.ones((S, n_cols, n)), 5.0 * (np.arange(S).reshape(S, 1) + 1) + 10000.0 * np.arange(n).reshape(1, n), tv


def _column(x):
    return np.array(x, dtype=np.float64).reshape(-1, 1)


def test_record_the_priming_sample_never_fires_and_the_window_is_the_samples_around_the_trigger():
    from nuclear_sim_amd import eventwin
    #         s = 0    1    2    3    4    5    6    7    8    9
    values, clock, tv = _series(_column([9.0, 9.0, 9.0, 0.0, 0.0, 9.0, 9.0, 9.0, 9.0, 9.0]))
    r = eventwin.record(values, clock, tv, [(">", 5.0)], 2, 1)
    assert r["plant"].tolist() == [0] and r["step"].tolist() == [5]      # beyond from the very first sample: that one only primes
    assert r["n_pre"].tolist() == [2] and r["n_post"].tolist() == [1] and r["flags"].tolist() == [0] and r["early"].tolist() == [False]
    assert r["trigger"].tolist() == [0] and r["fired"].tolist() == [1] and r["retriggers"].tolist() == [0] and r["episode"].tolist() == [0]
    assert r["time"].tolist() == [30.0] and r["times"].tolist() == [[20.0, 25.0, 30.0, 35.0]]
    assert r["values"].tolist() == [[[3.0, 103.0], [4.0, 104.0], [5.0, 105.0], [6.0, 106.0]]]
    assert r["values"].dtype == np.float64 and r["plant"].dtype == np.int32 and r["fired"].dtype == np.uint32
    # a single sample primes and nothing else
    assert len(eventwin.record(values[:1], clock[:1], tv[:1], [(">", 5.0)], 2, 1)["plant"]) == 0
    e = eventwin.record(values[:3], clock[:3], tv[:3], [(">", 5.0)], 2, 1)
    assert e["values"].shape == (0, 4, 2) and e["times"].shape == (0, 4) and e["early"].dtype == np.bool_


def test_record_beyond_is_edge_only_crossed_left_and_crossed_again_gives_two_records():
    from nuclear_sim_amd import eventwin
    #                          s = 0     1     2     3     4     5     6     7     8     9    10
    values, clock, tv = _series(_column([60.0, 49.0, 48.0, 47.0, 55.0, 50.0, 46.0, 45.0, 70.0, 70.0, 70.0]))
    r = eventwin.record(values, clock, tv, [("<", 50.0)], 1, 1)
    assert r["step"].tolist() == [1, 6]          # 50.0 itself is not beyond; staying beyond (2, 3, 7) does not fire again
    assert r["retriggers"].tolist() == [0, 0] and r["n_pre"].tolist() == [1, 1] and r["n_post"].tolist() == [1, 1]
    assert r["values"][:, :, 0].tolist() == [[0.0, 1.0, 2.0], [5.0, 6.0, 7.0]]
    up = eventwin.record(values, clock, tv, [(">", 50.0)], 0, 0)
    assert up["step"].tolist() == [4, 8] and up["values"].shape == (2, 1, 2)      # 60 at the priming sample does not count


def test_record_a_nan_never_fires_increase_and_bits_rise_looks_at_the_mask_only():
    from nuclear_sim_amd import eventwin
    nan = float("nan")
    #                          s = 0    1    2    3    4    5    6    7    8
    values, clock, tv = _series(_column([1.0, nan, 5.0, 5.0, 4.0, nan, nan, 4.5, 4.5]))
    r = eventwin.record(values, clock, tv, [("increase",)], 0, 0)
    assert r["step"].tolist() == []              # 1 -> NaN, NaN -> 5, 4 -> NaN, NaN -> 4.5: a NaN on either side
    values, clock, tv = _series(_column([1.0, nan, 5.0, 6.0, 6.0, 7.0, 3.0, 3.5, 3.5]))
    assert eventwin.record(values, clock, tv, [("increase",)], 0, 0)["step"].tolist() == [3, 5, 7]
    values, clock, tv = _series(_column([4.0, 5.0, 7.0, 3.0, 1.0, 9.0, -1.0, -1.0, 0.0]))
    r = eventwin.record(values, clock, tv, [("bits", 0x6)], 0, 0)
    assert r["step"].tolist() == [2, 6]          # bit 0 and bit 3 are outside the mask; bit 1 rises at 2; -1 has every bit; bit 2 set at 3 was set at 2
    both = eventwin.record(values, clock, np.concatenate([tv, tv], axis=1), [("bits", 0x8), ("bits", 0x6)], 0, 0)
    assert both["step"].tolist() == [2, 5, 6] and both["fired"].tolist() == [2, 1, 2] and both["trigger"].tolist() == [1, 0, 1]
    two = eventwin.record(values, clock, np.concatenate([tv, tv], axis=1), [("bits", 0x2), ("bits", 0x6)], 0, 0)
    assert two["fired"].tolist() == [3, 3] and two["trigger"].tolist() == [0, 0]      # the lowest trigger that fired, and the whole set


def test_record_n_pre_is_short_near_the_start_and_the_padding_is_exactly_outside_the_window():
    from nuclear_sim_amd import eventwin
    values, clock, tv = _series(np.array([[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 0, 0], [1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0]]))
    r = eventwin.record(values, clock, tv, [(">", 0.5)], 3, 2)
    assert r["plant"].tolist() == [0, 1, 2] and r["step"].tolist() == [1, 2, 4] and r["n_pre"].tolist() == [1, 2, 3] and r["n_post"].tolist() == [2, 2, 2]
    for i in range(3):
        pre, n_pre, n_post = 3, int(r["n_pre"][i]), int(r["n_post"][i])
        inside = (np.arange(6) >= pre - n_pre) & (np.arange(6) <= pre + n_post)
        assert np.array_equal(np.isnan(r["times"][i]), ~inside) and np.array_equal(np.isnan(r["values"][i]), np.repeat(~inside, 2).reshape(6, 2))
        assert r["values"][i, pre, 0] == 1000.0 * r["plant"][i] + r["step"][i] and r["times"][i, pre] == r["time"][i]      # row `pre` is the trigger sample
        assert np.array_equal(r["values"][i, inside, 1], 100.0 + 1000.0 * r["plant"][i] + np.arange(r["step"][i] - n_pre, r["step"][i] + n_post + 1))
    assert np.array_equal(r["values"][0].view(np.int64)[0], np.full(2, 0x7ff8000000000000))      # the NaN the device stores


def test_record_a_retrigger_while_armed_is_counted_and_not_recorded():
    from nuclear_sim_amd import eventwin
    #                          s = 0  1  2  3  4  5  6  7  8  9 10 11
    values, clock, tv = _series(_column([0, 1, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0]))
    r = eventwin.record(values, clock, tv, [(">", 0.5)], 1, 3)
    assert r["step"].tolist() == [1, 5] and r["retriggers"].tolist() == [1, 0]      # 3 falls into the first capture; 5 is after it (taken at 4); 9 is not due yet
    assert r["n_post"].tolist() == [3, 3]


def test_record_an_early_capture_at_an_episode_end_and_a_restart_empties_the_ring():
    from nuclear_sim_amd import eventwin
    #            s = 0  1  2  3  4  5  6  7  8  9 10 11
    trig = _column([0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0])
    ended = _column([0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0]).astype(bool)
    index = _column([0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2]).astype(np.int32)
    values, clock, tv = _series(trig)
    r = eventwin.record(values, clock, tv, [(">", 0.5)], 4, 3, ended=ended, episode_index=index)
    assert r["step"].tolist() == [3, 6] and r["episode"].tolist() == [0, 1]
    assert r["n_post"].tolist() == [1, 3] and r["flags"].tolist() == [1, 0] and r["early"].tolist() == [True, False]      # 4 ends the episode: early; 9 is due
    assert r["n_pre"].tolist() == [3, 1]                 # the second: the ring held only sample 5 of the new episode
    assert np.isnan(r["values"][0, 6:]).all() and not np.isnan(r["values"][0, 1:6]).any() and np.isnan(r["values"][0, 0]).all()
    assert r["values"][1, :, 0].tolist()[3:] == [5.0, 6.0, 7.0, 8.0, 9.0] and np.isnan(r["values"][1, :3]).all()
    # the end on the due step itself is no early capture; and an armed capture is dropped by a restart that is no episode end (abandoned)
    r = eventwin.record(values, clock, tv, [(">", 0.5)], 4, 1, ended=ended, episode_index=index)
    assert r["step"].tolist() == [3, 6] and r["flags"].tolist() == [0, 0] and r["n_post"].tolist() == [1, 1]
    r = eventwin.record(values, clock, tv, [(">", 0.5)], 4, 3, ended=None, episode_index=index)
    assert r["step"].tolist() == [6]
    # the first sample after a restart only primes: a trigger column that is beyond from the restart on does not fire
    trig2 = _column([0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1])
    values, clock, tv = _series(trig2)
    assert eventwin.record(values, clock, tv, [(">", 0.5)], 1, 1, episode_index=index)["step"].tolist() == []
    assert eventwin.record(values, clock, tv, [(">", 0.5)], 1, 1)["step"].tolist() == [5]


def test_record_orders_by_capture_step_then_plant():
    from nuclear_sim_amd import eventwin
    trig = np.zeros((10, 4))
    trig[2:, 3] = 1; trig[2:, 1] = 1; trig[4:, 0] = 1; trig[3:, 2] = 1
    ended = np.zeros((10, 4), dtype=bool); ended[4, 2] = True           # plant 2: triggered at 3, cut short at 4
    values, clock, tv = _series(trig)
    r = eventwin.record(values, clock, tv, [(">", 0.5)], 1, 3, ended=ended)
    assert r["plant"].tolist() == [2, 1, 3, 0] and (r["step"] + r["n_post"]).tolist() == [4, 5, 5, 7] and r["step"].tolist() == [3, 2, 2, 4]
    from nuclear_sim_amd.eventwin import same
    same(r, r)
    other = {k: v.copy() for k, v in r.items()}
    other["values"][1, 0, 0] = np.nan
    with pytest.raises(AssertionError, match="values differs"):
        same(other, r)
    with pytest.raises(ValueError):
        eventwin.record(values, clock, tv, [("sometimes",)], 1, 1)
    with pytest.raises(ValueError):
        eventwin.record(values, clock, tv, [(">", 0.5)], 1000, 24)
