"""CPU: the normaliser -- npb_set_normalizer and its companions -- is declared by include/npb.h, exported by libnpb.so and bound; the
binding lays the descriptor out as a C compiler does (a small compiled probe prints sizeof and every offsetof); the library's own check,
which needs no handle and reads no device memory, accepts a valid descriptor and names every refusal the header lists.  No compute calls.

The header keeps NPB_VERSION where the suites of the entry-point groups before this one pin it: the new entry points are detected by name."""
import ctypes

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

ENTRY_POINTS = ("npb_set_normalizer", "npb_normalizer_check", "npb_normalizer_training", "npb_normalizer_get_state", "npb_normalizer_set_state",
                "npb_normalizer_clear")
A16 = 0x7000       # "device addresses" the check only looks at: never dereferenced
F64, I32 = 0, 1    # NPB_KIND_*
NAN, INF = float("nan"), float("inf")


def test_header_declares_the_entry_points_and_the_rules_of_the_road():
    text = abi.header_text()
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_VERSION") == 154
    for words in ("a sample counts iff q - q == 0.0", "mean = shift + s1 / N", "M2 = (M2 + s2) - (s1 * s1) / N", "a bad value never poisons a statistic",
                  "ret * gamma rounded before the sum", "the mean is not subtracted", "Fresh frames", "set the normaliser first",
                  "Not here: statistics over fresh frames", "an exponential-moving-average variant", "normalizer.merge is the host answer",
                  # the tails of the sections that used to name this as missing now point here, and keep what their own suites pin
                  "Running statistics updated on the device have the normaliser's section below", "Not here: the terminal stack in the episode records",
                  "Running normalisation across\n * rollouts has the normaliser's section below", "gathering final_obs"):
        assert words in text, words


def test_library_exports_and_binding_declares_them():
    nine = [None] * 9
    abi.check_entry_points(ENTRY_POINTS, [("npb_set_normalizer", None, None), ("npb_normalizer_training", None, 1), ("npb_normalizer_clear", None, None, None),
                                          ("npb_normalizer_get_state", *nine), ("npb_normalizer_set_state", *nine)])


def test_the_binding_lays_the_descriptor_out_as_the_compiler_does():
    structs = {"npb_normalizer_desc_t": _lib.NpbNormalizerDesc}
    assert abi.probe(structs)[0] == abi.layout(structs)


class _Desc:
    """valid features -- an affine member column, an affine source, BITS on an int32 member, an affine source against a second column --
    and a valid normaliser on columns 0 and 1 with the return stream"""

    def __init__(self):
        from nuclear_sim_amd.schema import SCHEMA
        self.lib = _lib
        level = SCHEMA.slot("pump.oil_level", 1)[1]
        count = SCHEMA.slot("maint.maintenance_actions_performed")[1]
        self.cols = (_lib.NpbFeatureColumn * 4)()
        for F in self.cols:
            F.column.kind, F.column.slot, F.scale, F.lo, F.hi, F.nan_to = F64, level, 1.0, -INF, INF, NAN
        self.source(self.cols[1].column)
        self.cols[2].column.kind, self.cols[2].column.slot, self.cols[2].kind, self.cols[2].mask = I32, count, _lib.FEATURE_KINDS["bits"], 3
        self.source(self.cols[3].column)
        self.cols[3].ref_from_column = 1
        self.cols[3].ref_column.kind, self.cols[3].ref_column.slot = F64, level
        self.f = _lib.NpbFeaturesDesc()
        self.f.n_columns, self.f.columns, self.f.stack, self.f.out_type = 4, self.cols, 4, _lib.FEATURE_DTYPES["float32"]
        self.f.out, self.f.final = A16, None
        self.idx = (ctypes.c_int * 64)(0, 1)
        self.d = _lib.NpbNormalizerDesc()
        self.d.n_columns, self.d.columns, self.d.eps = 2, self.idx, 1e-8
        self.d.reward, self.d.gamma, self.d.clip, self.d.norm_reward = 1, 0.99, 5.0, A16 + 8
        self.features = True

    def source(self, C):
        C.from_source = 1
        C.source.base, C.source.type, C.source.rows, C.source.row_stride, C.source.plant_stride = A16, self.lib.SAMPLE_TYPES["f64"], 1, 0, 1


def _why(D, n=70):
    return abi.why(abi.library().npb_normalizer_check, ctypes.byref(D.d), n, ctypes.byref(D.f) if D.features else None)


def test_the_check_accepts_valid_normalisers_and_null():
    assert _why(_Desc()) is None
    assert abi.library().npb_normalizer_check(None, 70, None) is None
    D = _Desc(); D.d.reward, D.d.norm_reward, D.d.gamma, D.d.clip = 0, None, NAN, NAN      # columns alone: the return's members are not looked at
    assert _why(D) is None
    D = _Desc(); D.d.n_columns, D.d.columns, D.features = 0, None, False      # the return stream alone needs no features
    assert _why(D) is None
    D = _Desc(); D.d.eps, D.d.gamma = 0.0, 0.0
    assert _why(D) is None
    D = _Desc(); D.d.gamma = 1.0; D.d.clip = INF
    assert _why(D) is None


_set, _both = abi.set_path, abi.both


REFUSALS = [
    ("n_plants", None, "n_plants must be >= 1"),
    ("columns without features", _set(("features",), False), "columns chosen while no features are set"),
    ("too many columns", _set(("d", "n_columns"), 65), "column count must be 0 .. NPB_FEATURES_COLS_MAX (64)"),
    ("a negative count", _set(("d", "n_columns"), -1), "column count must be 0 .. NPB_FEATURES_COLS_MAX (64)"),
    ("columns without their array", _set(("d", "columns"), None), "with their indices"),
    ("index out of range", _set(("idx", 1), 4), "a column index out of range"),
    ("a negative index", _set(("idx", 0), -1), "a column index out of range"),
    ("a duplicate", _set(("idx", 1), 0), "a column named twice"),
    ("a BITS column", _set(("idx", 1), 2), "a NPB_FEATURE_BITS column"),
    ("a column-ref column", _set(("idx", 0), 3), "whose ref is a second column"),
    ("NaN eps", _set(("d", "eps"), NAN), "eps must be >= 0"),
    ("negative eps", _set(("d", "eps"), -1e-12), "eps must be >= 0"),
    ("gamma above 1", _set(("d", "gamma"), 1.0000001), "gamma must lie in [0, 1]"),
    ("negative gamma", _set(("d", "gamma"), -0.1), "gamma must lie in [0, 1]"),
    ("NaN gamma", _set(("d", "gamma"), NAN), "gamma must lie in [0, 1]"),
    ("NaN clip", _set(("d", "clip"), NAN), "clip must be positive"),
    ("clip 0", _set(("d", "clip"), 0.0), "clip must be positive"),
    ("negative clip", _set(("d", "clip"), -5.0), "clip must be positive"),
    ("NULL norm_reward", _set(("d", "norm_reward"), None), "a NULL norm_reward"),
    ("misaligned norm_reward", _set(("d", "norm_reward"), A16 + 4), "a misaligned norm_reward"),
    ("neither columns nor reward", _both(_set(("d", "n_columns"), 0), _set(("d", "reward"), 0)), "neither columns nor reward"),
]


@pytest.mark.parametrize("what, change, reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_check_names_every_refusal(what, change, reason):
    abi.check_refusal(_Desc, _why, "npb_set_normalizer: ", what, change, reason)


def test_features_the_library_would_refuse_are_refused_as_theirs():
    D = _Desc()
    D.f.stack = 0
    assert _why(D).startswith("npb_set_features: ")
