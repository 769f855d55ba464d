"""CPU: the column statistics (npb_set_column_stats, npb_column_stats_check, npb_column_stats_fold, npb_column_stats_clear,
npb_set_episode_record_stats) are declared by include/npb.h, exported by libnpb.so and bound, the binding laying both descriptors out as a C
compiler does; the library's own check, which needs no handle and reads no device memory, accepts a good descriptor and names every
refusal; the request builder of the binding refuses unknown names, indices and statistics before any device work; and colstats.fold, the
numpy statement of what the device folds, on hand-made series: the NaN rule, a limit crossed twice, the empty values, the moments.
No compute calls."""
import ctypes

import numpy as np
import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

ENTRY_POINTS = ("npb_set_column_stats", "npb_column_stats_check", "npb_column_stats_fold", "npb_column_stats_clear", "npb_set_episode_record_stats")
TABLES = ("min", "max", "sum", "sumsq", "last", "first_beyond", "n_beyond", "n_samples")
STATS_FIELDS = ("n_fields", "kinds", "slots", "n_sources", "sources", "direction", "limit") + TABLES
RECORD_FIELDS = TABLES + ("clear",)


@pytest.fixture(scope="module")
def L():
    return abi.library()


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_the_five_entry_points_and_keeps_the_version():
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_VERSION") == 154
    assert abi.define("NPB_COLUMN_STATS_MAX") == 32


def test_library_exports_and_binding_declares_them(L):
    from nuclear_sim_amd import colstats
    abi.check_entry_points(ENTRY_POINTS, [("npb_set_column_stats", None, None), ("npb_column_stats_fold", None, None),
                                          ("npb_column_stats_clear", None, None, None), ("npb_set_episode_record_stats", None, None)])
    assert L.npb_version() == 154
    assert _lib.COLUMN_STATS == colstats.STATS and _lib.COLUMN_STATS_MAX == colstats.MAX_COLUMNS == 32


def test_the_binding_lays_both_descriptors_out_as_the_compiler_does():
    A, B = _lib.NpbColumnStatsDesc, _lib.NpbEpisodeRecordStatsDesc
    assert tuple(f[0] for f in A._fields_) == STATS_FIELDS
    assert tuple(f[0] for f in B._fields_) == RECORD_FIELDS
    got = abi.probe({"npb_column_stats_desc_t": A, "npb_episode_record_stats_desc_t": B})[0]
    k = 1 + len(STATS_FIELDS)
    assert got[0] == ctypes.sizeof(A) and got[1:k] == [getattr(A, f).offset for f in STATS_FIELDS]
    assert got[k] == ctypes.sizeof(B) and got[k + 1:] == [getattr(B, f).offset for f in RECORD_FIELDS]


def _good(n_fields=2, n_sources=2, limits=((0, -1, 50.0), (3, 1, 1000.0))):
    """a descriptor the check accepts (it reads no device memory: the addresses only have to be aligned), and what keeps it alive"""
    from nuclear_sim_amd.schema import SCHEMA
    d = _lib.NpbColumnStatsDesc()
    members = [SCHEMA.slot("pump.oil_level", 0), SCHEMA.slot("maint.maintenance_actions_performed")][:n_fields]
    members += [SCHEMA.slot("pump.oil_level", 1)] * (n_fields - len(members))
    kinds = (ctypes.c_int * max(n_fields, 1))(*[0 if k == "f64" else 1 for k, _ in members])
    slots = (ctypes.c_int * max(n_fields, 1))(*[s for _, s in members])
    side = (_lib.NpbSampleSource * max(n_sources, 1))()
    for k in range(n_sources):
        side[k].base, side[k].type, side[k].rows, side[k].row_stride, side[k].plant_stride = 0x10000 + 64 * k, 0, 1, 0, 17
    n_cols = n_fields + n_sources
    direction, limit = (ctypes.c_int * max(n_cols, 1))(), (ctypes.c_double * max(n_cols, 1))()
    for c, dr, v in limits:
        direction[c], limit[c] = dr, v
    d.n_fields, d.kinds, d.slots, d.n_sources, d.sources, d.direction, d.limit = n_fields, kinds, slots, n_sources, side, direction, limit
    for j, name in enumerate(TABLES):
        setattr(d, name, 0x200000 + 0x1000 * j)
    return d, (kinds, slots, side, direction, limit)


def _why(L, d, n=70):
    r = L.npb_column_stats_check(ctypes.byref(d), n)
    return None if r is None else r.decode()


def test_check_accepts_a_good_descriptor(L):
    d, keep = _good()
    assert _why(L, d) is None
    assert L.npb_column_stats_check(None, 70) is None            # NULL = off
    d, keep = _good(limits=())                                    # no limits: fine without the limit tables
    d.first_beyond = d.n_beyond = None
    assert _why(L, d) is None
    d.direction = None; d.limit = None
    assert _why(L, d) is None
    for name in ("min", "max", "sum", "sumsq", "last"):         # any table but n_samples may be left out
        setattr(d, name, None)
    assert _why(L, d) is None
    d, keep = _good(n_fields=32, n_sources=0, limits=((0, 1, 0.0),))
    assert _why(L, d) is None
    d, keep = _good(n_fields=0, n_sources=1, limits=((0, 1, 0.0),))
    assert _why(L, d) is None


def test_check_names_every_refusal(L):
    def refused(change, word, **kw):
        d, keep = _good(**kw)
        change(d, keep)
        why = _why(L, d)
        assert why is not None and why.startswith("npb_set_column_stats:") and word in why, (word, why)

    refused(lambda d, k: None, "column count", n_fields=0, n_sources=0, limits=())
    refused(lambda d, k: None, "column count", n_fields=32, n_sources=1, limits=((0, 1, 0.0),))
    refused(lambda d, k: setattr(d, "n_fields", -1), "column count")
    refused(lambda d, k: k[0].__setitem__(0, 2), "bad field kind or slot")
    refused(lambda d, k: k[1].__setitem__(1, 1 << 20), "bad field kind or slot")
    refused(lambda d, k: k[1].__setitem__(0, -1), "bad field kind or slot")
    refused(lambda d, k: setattr(k[2][1], "base", None), "NULL base")
    refused(lambda d, k: setattr(k[2][0], "type", 4), "unknown element type")
    refused(lambda d, k: setattr(k[2][0], "type", -1), "unknown element type")
    refused(lambda d, k: setattr(k[2][0], "rows", 2), "rows == 1")
    refused(lambda d, k: setattr(k[2][0], "rows", 0), "rows == 1")
    refused(lambda d, k: k[3].__setitem__(1, 2), "direction outside")
    refused(lambda d, k: k[3].__setitem__(1, -2), "direction outside")
    refused(lambda d, k: k[4].__setitem__(0, float("nan")), "NaN limit")
    refused(lambda d, k: setattr(d, "n_samples", None), "n_samples must not be NULL")
    for name in TABLES[:6]:
        refused(lambda d, k, name=name: setattr(d, name, getattr(d, name) + 4), "misaligned table")
    refused(lambda d, k: setattr(d, "n_beyond", d.n_beyond + 2), "misaligned table")
    refused(lambda d, k: setattr(d, "n_samples", d.n_samples + 1), "misaligned table")
    refused(lambda d, k: None, "without a limit", limits=())
    refused(lambda d, k: setattr(d, "first_beyond", None), "without a limit", limits=())          # n_beyond alone
    refused(lambda d, k: setattr(d, "direction", None), "without a limit")


# ---------------------------------------------------------------------------------------------------------------- the request builder
def test_request_builder_orders_members_first_and_maps_the_limits():
    from nuclear_sim_amd.env import INFO_COLUMNS
    from nuclear_sim_amd.schema import SCHEMA
    req = _lib.column_stats_request(["reward", ("pump.oil_level", 1), ("info", "electrical_power"), "maint.maintenance_actions_performed", ("obs", 3)],
                                    limits={1: ("<", 40.0), 2: (">", 900.0)}, stats=("n_beyond", "min", "first_beyond"))
    assert req["members"] == [(0, SCHEMA.slot("pump.oil_level", 1)[1]), (1, SCHEMA.slot("maint.maintenance_actions_performed")[1])]
    assert req["sides"] == [("reward", 0, 1), ("info", INFO_COLUMNS.index("electrical_power"), len(INFO_COLUMNS)), ("obs", 3, 22)]
    assert req["order"] == [2, 0, 3, 1, 4]
    assert req["direction"] == [-1, 0, 0, 1, 0] and req["limit"] == [40.0, 0.0, 0.0, 900.0, 0.0]
    assert req["stats"] == ("min", "first_beyond", "n_beyond")                  # descriptor order
    assert _lib.column_stats_request(["pump.oil_level"])["stats"] == ("min", "max", "sum", "sumsq", "last")


@pytest.mark.parametrize("columns, limits, stats, word", [
    (["pump.no_such_member"], None, ("min",), "unknown column"),
    ([("pump.oil_level", 99)], None, ("min",), "no such instance"),
    ([("info", "no_such_column")], None, ("min",), "unknown info column"),
    ([("obs", 22)], None, ("min",), "unknown obs column"),
    ([("obs", -1)], None, ("min",), "unknown obs column"),
    (["pump.oil_level"], None, ("median",), "unknown statistic"),
    (["pump.oil_level"], {1: ("<", 1.0)}, ("min",), "limit on column"),
    (["pump.oil_level"], {0: ("<=", 1.0)}, ("min",), "must be ('>' | '<', value)"),
    (["pump.oil_level"], {0: ("<", float("nan"))}, ("min",), "NaN"),
    (["pump.oil_level"], None, ("min", "n_beyond"), "need a limit"),
    ([], None, ("min",), "1 to 32 columns"),
    (["reward"] * 33, None, ("min",), "1 to 32 columns"),
])
def test_request_builder_refuses(columns, limits, stats, word):
    with pytest.raises(ValueError) as e:
        _lib.column_stats_request(columns, limits, stats)
    assert word in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------------- colstats.fold
def test_fold_empty_values():
    from nuclear_sim_amd import colstats
    s = colstats.fold(np.zeros((0, 2, 3)), np.zeros((0, 3)), limits={0: ("<", 1.0)})
    assert np.all(s["min"] == np.inf) and np.all(s["max"] == -np.inf) and np.all(s["sum"] == 0) and np.all(s["sumsq"] == 0)
    assert np.isnan(s["last"]).all() and np.all(s["first_beyond"] == np.inf) and np.all(s["n_beyond"] == 0) and np.all(s["n_samples"] == 0)
    assert s["n_beyond"].dtype == s["n_samples"].dtype == np.int32 and s["min"].shape == (2, 3) and s["n_samples"].shape == (3,)
    mean, var = colstats.moments(s)
    assert np.isnan(mean).all() and np.isnan(var).all()


def test_fold_nan_rule_and_sequential_sums():
    from nuclear_sim_amd import colstats
    series = np.array([3.0, np.nan, 1.0, 0.1, 0.2, 1e16, 1.0, -1e16])
    s = colstats.fold(series.reshape(-1, 1, 1), np.arange(8.0).reshape(-1, 1))
    assert s["min"][0, 0] == -1e16 and s["max"][0, 0] == 1e16                 # a NaN sample replaces neither
    assert np.isnan(s["sum"][0, 0]) and np.isnan(s["sumsq"][0, 0]) and s["last"][0, 0] == -1e16 and s["n_samples"][0] == 8
    # a NaN first and last: min / max keep what they had; last takes it
    s = colstats.fold(np.array([np.nan, 2.0, np.nan]).reshape(-1, 1, 1), np.zeros((3, 1)))
    assert s["min"][0, 0] == 2.0 and s["max"][0, 0] == 2.0 and np.isnan(s["last"][0, 0])
    s = colstats.fold(np.array([np.nan]).reshape(-1, 1, 1), np.zeros((1, 1)))
    assert s["min"][0, 0] == np.inf and s["max"][0, 0] == -np.inf
    # the sums are the sequential ones, in step order: not numpy's pairwise sum, not the exactly rounded one
    v = np.array([0.1, 0.2, 0.3, 1e16, 1.0, -1e16, 0.7])
    s = colstats.fold(v.reshape(-1, 1, 1), np.zeros((7, 1)))
    acc = acc2 = 0.0
    for x in v:
        acc = acc + x
        acc2 = acc2 + x * x
    assert s["sum"][0, 0] == acc and s["sumsq"][0, 0] == acc2 and acc != float(np.sum(np.sort(v)))
    # `into` goes on from tables: two halves equal the whole
    a = colstats.fold(v[:3].reshape(-1, 1, 1), np.zeros((3, 1)))
    b = colstats.fold(v[3:].reshape(-1, 1, 1), np.zeros((4, 1)), into=a)
    colstats.same(b, s)


def test_fold_a_limit_crossed_left_and_crossed_again():
    from nuclear_sim_amd import colstats
    #                 t =  5    10    15    20    25    30    35
    low = np.array([60.0, 49.0, 48.0, 55.0, 50.0, 47.0, 70.0])        # '<' 50: beyond at 10, 15, 30 (50.0 itself is not)
    high = np.array([1.0, 2.0, 3.0, 2.0, 3.5, 1.0, 3.0])              # '>' 3: beyond at 25 only (3.0 itself is not)
    never = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])             # '>' 3: never
    values = np.array([[low, low + 100.0], [high, never], [low, low]]).transpose(2, 0, 1)      # [7 steps, 3 columns, 2 plants]
    times = np.stack([5.0 * np.arange(1, 8), 1000.0 + 5.0 * np.arange(1, 8)], axis=1)
    s = colstats.fold(values, times, limits={0: ("<", 50.0), 1: (">", 3.0)})
    assert s["first_beyond"].tolist() == [[10.0, np.inf], [25.0, np.inf], [np.inf, np.inf]]      # the first crossing; no limit = never
    assert s["n_beyond"].tolist() == [[3, 0], [1, 0], [0, 0]]                                      # both visits counted
    assert s["n_samples"].tolist() == [7, 7] and s["min"][0, 0] == 47.0 and s["last"][0, 0] == 70.0 and s["min"][0, 0] < s["last"][0, 0]
    with pytest.raises(ValueError):
        colstats.fold(values, times, limits={3: ("<", 1.0)})
    with pytest.raises(ValueError):
        colstats.fold(values, times, limits={0: ("<", float("nan"))})


def test_moments():
    from nuclear_sim_amd import colstats
    rng = np.random.default_rng(3)
    v = rng.normal(40.0, 3.0, size=(50, 2, 4))
    s = colstats.fold(v, np.zeros((50, 4)))
    mean, var = colstats.moments(s)
    assert np.allclose(mean, v.mean(axis=0), rtol=1e-13) and np.allclose(var, v.var(axis=0), rtol=1e-9)
    const = colstats.fold(np.full((9, 1, 1), 0.1), np.zeros((9, 1)))      # rounding can take sumsq / k below mean^2: the variance is not negative
    assert colstats.moments(const)[1][0, 0] >= 0.0
