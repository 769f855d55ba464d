"""CPU: features -- the caller's policy inputs (npb_set_features and its companions) -- are declared by include/npb.h, exported by
libnpb.so and bound; the binding lays the descriptors out as a C compiler does (a small compiled probe prints sizeof and every offsetof);
the library's own check, which needs no handle and reads no device memory, accepts a valid descriptor and names every refusal the header
lists.  No compute calls.

The header keeps NPB_VERSION where the suites of the entry-point groups before this one pin it: the new entry points are detected by name."""
import ctypes
import re

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

ENTRY_POINTS = ("npb_set_features", "npb_features_check", "npb_features_prime", "npb_features_clear", "npb_features_get_state",
                "npb_features_set_state")
STRUCTS = {"npb_feature_column_t": _lib.NpbFeatureColumn, "npb_features_desc_t": _lib.NpbFeaturesDesc}
A16 = 0x7000       # "device addresses" the check only looks at: never dereferenced
F64, I32 = 0, 1    # NPB_KIND_*
NAN, INF = float("nan"), float("inf")


def test_header_declares_the_entry_points_the_maxima_and_the_rules_of_the_road():
    text = abi.header_text()
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_FEATURES_COLS_MAX") == 64
    assert abi.define("NPB_FEATURES_STACK_MAX") == 16
    assert abi.define("NPB_FEATURES_CELLS_MAX") == 256
    assert abi.define("NPB_VERSION") == 154
    for words in ("rounded before the product", "a NaN passes both comparisons", "overflows to an infinity", "THE quiet NaN", "the terminal frame pass A just",
                  "No half types", "Not here: the terminal stack in the episode records"):
        assert words in text, words


def test_library_exports_and_binding_declares_them():
    abi.check_entry_points(ENTRY_POINTS, [("npb_set_features", None, None), ("npb_features_prime", None, None),
                                          ("npb_features_clear", None, None, None), ("npb_features_get_state", None, None, None, None),
                                          ("npb_features_set_state", None, None, None, None)])


def test_the_binding_lays_the_descriptors_out_as_the_compiler_does():
    from nuclear_sim_amd import features
    # the initialiser macros name the members kind, mask
    c, a = "((npb_feature_column_t){ {0}, NPB_FEATURE_BITS(0xF00) })", "((npb_feature_column_t){ {0}, NPB_FEATURE_AFFINE })"
    got, values = abi.probe(STRUCTS, [c + ".kind", c + ".mask", a + ".kind", a + ".mask"])
    assert got == abi.layout(STRUCTS)
    assert values == [_lib.FEATURE_KINDS["bits"], 0xF00, _lib.FEATURE_KINDS["affine"], 0]
    text = abi.header_text()
    assert {name: int(re.search(r"NPB_FEATURE_KIND_%s = (\d+)" % name.upper(), text).group(1)) for name in _lib.FEATURE_KINDS} == _lib.FEATURE_KINDS
    assert {"float32": int(re.search(r"NPB_FEATURES_F32 = (\d+)", text).group(1)),
            "float64": int(re.search(r"NPB_FEATURES_F64 = (\d+)", text).group(1))} == _lib.FEATURE_DTYPES
    assert tuple(_lib.FEATURE_KINDS) == features.KINDS and tuple(_lib.FEATURE_DTYPES) == features.DTYPES
    assert (_lib.FEATURES_COLS_MAX, _lib.FEATURES_STACK_MAX, _lib.FEATURES_CELLS_MAX) == (features.COLS_MAX, features.STACK_MAX, features.CELLS_MAX) == (64, 16, 256)


class _Desc:
    """a valid descriptor: an affine member column, an affine source against a second (member) column, BITS on an int32 member and on a
    u8 source, float output with a final tensor; and the ctypes array it points into"""

    def __init__(self):
        from nuclear_sim_amd.schema import SCHEMA
        self.lib = _lib
        level = SCHEMA.slot("pump.oil_level", 1)[1]
        count = SCHEMA.slot("maint.maintenance_actions_performed")[1]
        self.cols = (_lib.NpbFeatureColumn * 64)()
        for F in self.cols:
            F.column.kind, F.column.slot, F.scale, F.lo, F.hi, F.nan_to = F64, level, 1.0, -INF, INF, NAN
        self.cols[0].scale, self.cols[0].ref, self.cols[0].lo, self.cols[0].hi = 0.01, 50.0, -1.0, 1.0
        self.source(self.cols[1].column, "f64")
        self.cols[1].ref_from_column = 1
        self.cols[1].ref_column.kind, self.cols[1].ref_column.slot = F64, level
        self.cols[2].column.kind, self.cols[2].column.slot, self.cols[2].kind, self.cols[2].mask = I32, count, _lib.FEATURE_KINDS["bits"], 3
        self.source(self.cols[3].column, "u8")
        self.cols[3].kind, self.cols[3].mask, self.cols[3].fresh = _lib.FEATURE_KINDS["bits"], 0xFF, 1.0
        self.d = _lib.NpbFeaturesDesc()
        self.d.n_columns, self.d.columns, self.d.stack, self.d.out_type = 4, self.cols, 4, _lib.FEATURE_DTYPES["float32"]
        self.d.out, self.d.final = A16, A16 + 4

    def source(self, C, kind):
        C.from_source = 1
        C.source.base, C.source.type, C.source.rows, C.source.row_stride, C.source.plant_stride = A16, self.lib.SAMPLE_TYPES[kind], 1, 0, 1


def _why(D, n=70):
    return abi.why(abi.library().npb_features_check, ctypes.byref(D.d), n)


def test_the_check_accepts_valid_features_and_null():
    assert _why(_Desc()) is None
    assert abi.library().npb_features_check(None, 70) is None
    D = _Desc(); D.d.final = None                                  # optional
    assert _why(D) is None
    D = _Desc(); D.d.n_columns, D.d.stack = 64, 4                  # the largest shape: 256 cells
    assert _why(D) is None
    D = _Desc(); D.d.n_columns, D.d.stack = 16, 16
    assert _why(D) is None
    D = _Desc(); D.d.out_type, D.d.out, D.d.final = 1, A16 + 8, A16 + 16      # double
    assert _why(D) is None
    D = _Desc(); D.cols[0].scale = INF; D.cols[0].nan_to = 0.0; D.cols[0].lo = D.cols[0].hi = 2.0      # the caller's business
    assert _why(D) is None


_set, _both = abi.set_path, abi.both


REFUSALS = [
    ("n_plants", None, "n_plants must be >= 1"),
    ("no columns", _set(("d", "n_columns"), 0), "column count must be 1 .. NPB_FEATURES_COLS_MAX (64)"),
    ("too many columns", _both(_set(("d", "n_columns"), 65), _set(("d", "stack"), 1)), "column count must be 1 .. NPB_FEATURES_COLS_MAX (64)"),
    ("columns without their array", _set(("d", "columns"), None), "with their descriptors"),
    ("no stack", _set(("d", "stack"), 0), "stack depth must be 1 .. NPB_FEATURES_STACK_MAX (16)"),
    ("too deep a stack", _both(_set(("d", "stack"), 17), _set(("d", "n_columns"), 1)), "stack depth must be 1 .. NPB_FEATURES_STACK_MAX (16)"),
    ("too many cells", _both(_set(("d", "stack"), 8), _set(("d", "n_columns"), 33)), "stack * columns must be <= NPB_FEATURES_CELLS_MAX (256)"),
    ("bad kind of member", _set(("cols", 0, "column", "kind"), 7), "bad field kind or slot"),
    ("bad slot", _set(("cols", 0, "column", "slot"), 1 << 20), "bad field kind or slot"),
    ("bad slot of a ref column", _set(("cols", 1, "ref_column", "slot"), -3), "bad field kind or slot"),
    ("NULL base", _set(("cols", 1, "column", "source", "base"), None), "a side source has a NULL base"),
    ("unknown type", _set(("cols", 3, "column", "source", "type"), 9), "a side source has an unknown element type"),
    ("rows != 1", _set(("cols", 1, "column", "source", "rows"), 2), "a side source must have rows == 1"),
    ("unknown feature kind", _set(("cols", 0, "kind"), 2), "an unknown feature kind"),
    ("BITS on a real member", _set(("cols", 2, "column", "kind"), F64), "NPB_FEATURE_BITS on a real-valued column"),
    ("BITS on a real source", _set(("cols", 3, "column", "source", "type"), 0), "NPB_FEATURE_BITS on a real-valued column"),
    ("BITS with mask 0", _set(("cols", 2, "mask"), 0), "NPB_FEATURE_BITS with mask 0"),
    ("NaN scale", _set(("cols", 0, "scale"), NAN), "a NaN scale"),
    ("NaN ref", _set(("cols", 0, "ref"), NAN), "a NaN ref"),
    ("NaN lo", _set(("cols", 0, "lo"), NAN), "a NaN clip limit"),
    ("NaN hi", _set(("cols", 3, "hi"), NAN), "a NaN clip limit"),
    ("NaN fresh", _set(("cols", 3, "fresh"), NAN), "a NaN fresh value"),
    ("lo > hi", _both(_set(("cols", 0, "lo"), 2.0), _set(("cols", 0, "hi"), 1.0)), "a clip with lo > hi"),
    ("unknown out type", _set(("d", "out_type"), 2), "an unknown out type"),
    ("NULL out", _set(("d", "out"), None), "a NULL out tensor"),
    ("misaligned out", _set(("d", "out"), A16 + 2), "a misaligned tensor"),
    ("misaligned final", _set(("d", "final"), A16 + 6), "a misaligned tensor"),
    ("double out on 4 bytes", _both(_set(("d", "out_type"), 1), _set(("d", "final"), None), _set(("d", "out"), A16 + 4)), "a misaligned tensor"),
    ("double final on 4 bytes", _set(("d", "out_type"), 1), "a misaligned tensor"),
]


@pytest.mark.parametrize("what, change, reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_check_names_every_refusal(what, change, reason):
    abi.check_refusal(_Desc, _why, "npb_set_features: ", what, change, reason)


def test_scale_and_ref_are_read_only_where_the_kind_has_them():
    """scale and ref belong to AFFINE: a BITS column's are not looked at"""
    D = _Desc()
    D.cols[2].scale = NAN; D.cols[2].ref = NAN
    assert _why(D) is None
