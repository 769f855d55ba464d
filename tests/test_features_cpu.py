"""CPU: the numpy statement of the features (nuclear_sim_amd/features.py) against hand-computed frames, the stack's three passes over a
scripted sequence, the host-side request (``_lib.features_request``) and its refusals by name, and ``features.spec_from_stats``.  No
library, no device."""
import numpy as np
import pytest

from nuclear_sim_amd import _lib, features

NAN, INF = float("nan"), float("inf")


def _spec(columns, stack=1, dtype="float32"):
    return {"stack": stack, "dtype": dtype, "columns": columns}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------------------------------------ the transform
def test_nan_to_comes_before_the_clip():
    """a NaN replaced by 9 is then clipped to hi = 2; the other order would leave 9"""
    spec = _spec([features.column(0, nan_to=9.0, lo=-1.0, hi=2.0)])
    f = features.frame(np.array([[NAN, 0.5, -7.0]]), spec)
    assert f[:, 0].tolist() == [2.0, 0.5, -1.0]


def test_a_nan_passes_the_clip():
    spec = _spec([features.column(0, lo=-1.0, hi=2.0)])
    f = features.frame(np.array([[NAN, 5.0]]), spec)
    assert np.isnan(f[0, 0]) and f[1, 0] == 2.0


def test_inf_minus_inf_through_a_column_ref_on_itself():
    """v - v: 0 where v is finite, NaN where it is infinite; nan_to then names it"""
    rows = np.array([[INF, 3.0, -INF]])
    f = features.frame(rows, _spec([features.column(0, ref=("col", 0))], dtype="float64"))
    assert np.isnan(f[0, 0]) and f[1, 0] == 0.0 and np.isnan(f[2, 0])
    f = features.frame(rows, _spec([features.column(0, ref=("col", 0), nan_to=-1.0)], dtype="float64"))
    assert f[:, 0].tolist() == [-1.0, 0.0, -1.0]


def test_the_subtraction_is_rounded_before_the_product():
    """(v - ref) * scale with v - ref inexact: not v * scale - ref * scale, and not a fused form"""
    v, ref, scale = 0.1, 0.3, 3.0
    f = features.frame(np.array([[v]]), _spec([features.column(0, ref=ref, scale=scale)], dtype="float64"))
    assert f[0, 0] == (np.float64(v) - np.float64(ref)) * np.float64(scale)
    assert f[0, 0] != np.float64(v) * scale - np.float64(ref) * scale


def test_float32_rounds_a_halfway_value_to_even():
    """1 + 2^-24 lies halfway between 1 and 1 + 2^-23: to even is 1; 1 + 3 * 2^-24 lies halfway between 1 + 2^-23 and 1 + 2^-22: to even is
    the latter"""
    rows = np.array([[1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50]])
    f = features.frame(rows, _spec([features.column(0)]))
    assert f.dtype == np.float32
    assert _bits(f[:, 0]).tolist() == [0x3F800000, 0x3F800002, 0x3F800001]


def test_float32_keeps_subnormals_and_overflows_to_inf():
    rows = np.array([[1.0, 3.0, 1e300]])
    f = features.frame(rows, _spec([features.column(0, scale=2.0 ** -149)]))
    assert _bits(f[:2, 0]).tolist() == [1, 3] and f[2, 0] == np.float32(INF)      # 1e300 * 2^-149 is still beyond float32
    f = features.frame(np.array([[1.0]]), _spec([features.column(0, scale=2.0 ** -150)]))
    assert _bits(f[:, 0]).tolist() == [0]                                       # halfway between 0 and the least subnormal: to even


def test_bits():
    rows = np.array([[0.0, 0x100, 0x0FF, -1.0, 0xF00]])
    f = features.frame(rows, _spec([features.column(0, kind="bits", mask=0xF00)]))
    assert f[:, 0].tolist() == [0.0, 1.0, 0.0, 1.0, 1.0]


def test_fresh_values_for_side_columns():
    """in a fresh frame a live column is read, any other takes its fresh raw value through the same transform; a second column too"""
    cols = [features.column(0, live=True, scale=2.0),
            features.column(1, fresh=5.0, ref=1.0, scale=10.0),
            features.column(1, kind="bits", mask=4, fresh=6.0),
            features.column(0, live=True, ref=("col", 1), ref_fresh=0.5),
            features.column(1, ref=("col", 0), ref_live=True)]
    rows = np.array([[3.0, 4.0], [100.0, 200.0]])
    f = features.frame(rows, _spec(cols, dtype="float64"), fresh=True)
    assert f.tolist() == [[6.0, 40.0, 1.0, 2.5, -3.0], [8.0, 40.0, 1.0, 3.5, -4.0]]
    f = features.frame(rows, _spec(cols, dtype="float64"))
    assert f[0].tolist() == [6.0, 990.0, 1.0, -97.0, 97.0]


# ------------------------------------------------------------------------------------------------ the stack
def _rows(t, n=3):
    return np.array([[10.0 * t + p for p in range(n)], [-(10.0 * t + p) for p in range(n)]])


def test_shift_fill_restart_and_final_over_a_scripted_sequence():
    spec = _spec([features.column(0, live=True), features.column(1, fresh=7.0)], stack=3, dtype="float64")
    S = features.Stack(spec, 3, final=True, final_fill=-99.0)
    index = np.zeros(3, dtype=np.int32)
    assert S.step(_rows(0), index).all()                                   # unprimed: every slot filled
    assert S.out[1].tolist() == [[1.0, -1.0]] * 3
    assert not S.restart(_rows(0), index).any()
    assert not S.step(_rows(1), index).any()                                # primed, same episode: shift and append
    assert S.out[1].tolist() == [[1.0, -1.0], [1.0, -1.0], [11.0, -11.0]]
    S.step(_rows(2), index)
    assert S.out[2].tolist() == [[2.0, -2.0], [12.0, -12.0], [22.0, -22.0]]
    # step 3: plant 1 ends; the episode kernel restores it (its member row reads 500) and bumps its index
    S.step(_rows(3), index)
    index[1] += 1
    after = _rows(3); after[0, 1] = 500.0
    assert S.restart(after, index).tolist() == [False, True, False]
    assert S.final[1].tolist() == [[11.0, -11.0], [21.0, -21.0], [31.0, -31.0]]        # the stack that ended, terminal frame included
    assert np.all(S.final[0] == -99.0) and np.all(S.final[2] == -99.0)                  # the others' rows untouched
    assert S.out[1].tolist() == [[500.0, 7.0]] * 3                                      # K copies of the fresh frame: member live, side fresh
    assert S.out[0].tolist() == [[10.0, -10.0], [20.0, -20.0], [30.0, -30.0]]
    assert S.seen.tolist() == [0, 1, 0]
    assert not S.step(_rows(4), index).any()                                            # the restarted plant shifts from its fresh frames
    assert S.out[1].tolist() == [[500.0, 7.0], [500.0, 7.0], [41.0, -41.0]]
    # the caller restores plant 2 between two steps: its index changed, pass A fills
    index[2] += 1
    assert S.step(_rows(5), index).tolist() == [False, False, True]
    assert S.out[2].tolist() == [[52.0, -52.0]] * 3 and S.out[0][-1].tolist() == [50.0, -50.0]
    # clear, then prime: only the unprimed plant takes the fresh frame
    S.clear(np.array([True, False, False]))
    assert S.prime(_rows(6), index).tolist() == [True, False, False]
    assert S.out[0].tolist() == [[60.0, 7.0]] * 3 and S.out[1][-1].tolist() == [51.0, -51.0]
    assert not S.step(_rows(7), index).any()                                            # primed by the priming: shifts
    S.clear()
    assert S.step(_rows(8), index).all()                                                # cleared and stepped: fills


def test_without_an_index_nothing_restarts():
    spec = _spec([features.column(0, live=True)], stack=2)
    S = features.Stack(spec, 2)
    S.prime(_rows(1, 2))
    assert S.out[:, :, 0].tolist() == [[10.0, 10.0], [11.0, 11.0]] and S.primed.all()
    S.step(_rows(2, 2))
    assert S.out[:, :, 0].tolist() == [[10.0, 20.0], [11.0, 21.0]] and S.final is None


# ------------------------------------------------------------------------------------------------ the request
def test_the_request_resolves_words_and_options():
    req = _lib.features_request([("pump.oil_level", 1),
                                 (("info", "electrical_power"), {"scale": 0.001, "ref": 790.0, "clip": (-1.0, None), "nan_to": 0.0}),
                                 ("flags", {"bits": 0xF00, "fresh": 0x100}),
                                 (("obs", 5), {"ref": ("obs", 6)}),
                                 ("reward", {"ref": ("pump.oil_level", 1), "ref_fresh": 2.0}),
                                 ("pump.oil_level", 1)], stack=4, dtype="float64")
    spec, rows = req["spec"], req["columns"]
    assert spec["stack"] == 4 and spec["dtype"] == "float64" and len(spec["columns"]) == 6
    assert len(rows) == 6 and spec["columns"][0]["col"] == spec["columns"][5]["col"] == spec["columns"][4]["ref"][1]      # a word read twice is one row
    c = spec["columns"]
    assert c[0]["live"] and not c[1]["live"] and not c[2]["live"] and c[3]["live"] and c[3]["ref_live"] and not c[4]["live"] and c[4]["ref_live"]
    assert (c[1]["scale"], c[1]["ref"], c[1]["lo"], c[1]["hi"], c[1]["nan_to"]) == (0.001, 790.0, -1.0, INF, 0.0)
    assert c[2]["kind"] == "bits" and c[2]["mask"] == 0xF00 and c[2]["fresh"] == 256.0 and np.isnan(c[0]["nan_to"])
    assert rows[c[2]["col"]]["side"] == ("flags", 0, 1, "i32") and rows[c[0]["col"]]["member"] is not None
    features.check(spec)
    assert _lib.features_request(["reward"], dtype=np.float32)["spec"]["dtype"] == "float32"      # a numpy dtype; a lone word


REFUSALS = [
    (dict(columns=[]), "1 to 64 columns"),
    (dict(columns=["reward"] * 65), "1 to 64 columns"),
    (dict(columns=["reward"], stack=0), "stack depth"),
    (dict(columns=["reward"], stack=17), "stack depth"),
    (dict(columns=["reward"] * 33, stack=8), "stack * columns"),
    (dict(columns=["reward"], dtype="float16"), "float32 or float64"),
    (dict(columns=["no.such_member"]), "unknown column"),
    (dict(columns=[("info", "no_such")]), "unknown info column"),
    (dict(columns=[("obs", 22)]), "unknown obs column"),
    (dict(columns=["task_reward"]), "needs a task"),
    (dict(columns=[("work_order", 0)]), "enable_maintenance_summary"),
    (dict(columns=[("work_order", 3)], summary_keys=2), "keys are 0 .. 1"),
    (dict(columns=[("reward", {"gain": 2.0})]), "unknown option 'gain'"),
    (dict(columns=[("reward", {"bits": 1})]), "'bits' needs an integer column"),
    (dict(columns=[("flags", {"bits": 0})]), "0 < mask"),
    (dict(columns=[("flags", {"bits": 1, "scale": 2.0})]), "'bits' excludes"),
    (dict(columns=[("reward", {"scale": NAN})]), "the scale is NaN"),
    (dict(columns=[("reward", {"ref": NAN})]), "the ref is NaN"),
    (dict(columns=[("reward", {"ref": "no.such_member"})]), "unknown column"),
    (dict(columns=[("reward", {"clip": (2.0, 1.0)})]), "lo > hi"),
    (dict(columns=[("reward", {"clip": (NAN, 1.0)})]), "lower clip limit is NaN"),
    (dict(columns=[("reward", {"clip": 3.0})]), "'clip' is (lo, hi)"),
    (dict(columns=[("flags", {"fresh": NAN})]), "fresh is NaN"),
    (dict(columns=[("reward", {"scale": "x"})]), "must be a number"),
]


@pytest.mark.parametrize("kw, reason", REFUSALS, ids=[r[1] + str(i) for i, r in enumerate(REFUSALS)])
def test_the_request_refuses_by_name(kw, reason):
    with pytest.raises(ValueError) as e:
        _lib.features_request(**kw)
    assert reason in str(e.value), str(e.value)


def test_task_reward_with_a_task_and_summary_rows():
    req = _lib.features_request(["task_reward", ("completed", 1)], task=True, summary_keys=2)
    assert [R["side"][0] for R in req["columns"]] == ["task_reward", "n_completed"]


def test_check_refuses_what_the_device_would():
    for change, reason in (({"stack": 17}, "stack depth"), ({"dtype": "float16"}, "float32 or float64")):
        with pytest.raises(ValueError, match=reason):
            features.check(dict(_spec([features.column(0)]), **change))
    for col, reason in ((features.column(0, kind="rate"), "unknown kind"), (features.column(0, kind="bits"), "mask"),
                        (features.column(0, scale=NAN), "scale is NaN"), (features.column(0, lo=1.0, hi=0.0), "lo > hi"),
                        (features.column(0, fresh=NAN), "fresh is NaN")):
        with pytest.raises(ValueError, match=reason):
            features.check(_spec([col]))
    with pytest.raises(ValueError, match="stack \\* columns"):
        features.check(_spec([features.column(0)] * 33, stack=8))


# ------------------------------------------------------------------------------------------------ the normaliser
def test_spec_from_stats():
    """two plants, three samples in all of column 1: 1, 2, 6 -> mean 3, variance 41/3 - 9; column 0 is constant: scale 1"""
    stats = {"sum": np.array([[8.0, 4.0], [3.0, 6.0]]), "sumsq": np.array([[32.0, 16.0], [5.0, 36.0]]), "n_samples": np.array([2, 1])}
    got = features.spec_from_stats(stats, [1, 0])
    assert got[0]["ref"] == 3.0 and got[0]["scale"] == 1.0 / np.sqrt(41.0 / 3.0 - 9.0)
    assert got[1] == {"ref": 4.0, "scale": 1.0}
    req = _lib.features_request([("reward", got[0])])                       # the options set_features takes
    f = features.frame(np.array([[1.0, 2.0, 6.0]]), dict(req["spec"], dtype="float64"))[:, 0]
    assert abs(f.mean()) < 1e-15 and abs(f.std() - 1.0) < 1e-15
    with pytest.raises(ValueError, match="no sample"):
        features.spec_from_stats(dict(stats, n_samples=np.array([0, 0])), [0])


def test_a_nan_that_stays_is_the_quiet_nan():
    """inf - inf gives a NaN whose sign differs between machines: the statement fixes the bits, sign clear and no payload"""
    rows = np.array([[INF, -INF, NAN]])
    f = features.frame(rows, _spec([features.column(0, ref=("col", 0))], dtype="float64"))
    assert _bits(f[:, 0]).tolist() == [0x7FF8000000000000] * 3
    f = features.frame(rows, _spec([features.column(0, ref=("col", 0), lo=-1.0, hi=1.0)]))
    assert _bits(f[:, 0]).tolist() == [0x7FC00000] * 3
