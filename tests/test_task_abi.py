"""CPU: tasks -- caller-defined reward terms and termination rules (npb_set_task and its companions) -- are declared by include/npb.h,
exported by libnpb.so and bound; the binding lays the four descriptors out as a C compiler does (a small compiled probe prints sizeof and
every offsetof); the library's own check, which needs no handle and reads no device memory, accepts a valid descriptor and names every
refusal the header lists.  No compute calls.

The header keeps NPB_VERSION where the suites of the entry-point groups before this one pin it: the new entry points are detected by name."""
import ctypes
import re

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

ENTRY_POINTS = ("npb_set_task", "npb_task_check", "npb_task_clear", "npb_task_get_state", "npb_task_set_state", "npb_set_episode_record_task")
STRUCTS = {"npb_task_column_t": _lib.NpbTaskColumn, "npb_task_term_t": _lib.NpbTaskTerm, "npb_task_rule_t": _lib.NpbTaskRule, "npb_task_desc_t": _lib.NpbTaskDesc}
A8 = 0x7000        # "device addresses" the check only looks at: never dereferenced
F64, I32 = 0, 1    # NPB_KIND_*


def test_header_declares_the_entry_points_the_maxima_and_the_rules_of_the_road():
    text = abi.header_text()
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_TASK_TERMS_MAX") == 16
    assert abi.define("NPB_TASK_RULES_MAX") == 8
    assert abi.define("NPB_VERSION") == 154
    for words in ("A NaN sample gives a NaN reward", "LEVELS, not edges", "keeps reporting done", "each product rounded before its add"):
        assert words in text, words


def test_library_exports_and_binding_declares_them():
    abi.check_entry_points(ENTRY_POINTS, [("npb_set_task", None, None), ("npb_task_clear", None, None, None),
                                          ("npb_set_episode_record_task", None, None)])


def test_the_binding_lays_the_descriptors_out_as_the_compiler_does():
    assert abi.probe(STRUCTS)[0] == abi.layout(STRUCTS)
    text = abi.header_text()
    assert {name: int(re.search(r"NPB_TASK_%s = (\d+)" % name.upper(), text).group(1)) for name in _lib.TASK_KINDS} == _lib.TASK_KINDS
    assert {name: int(re.search(r"NPB_TASK_RULE_MODE_%s = (\d+)" % name.upper(), text).group(1)) for name in _lib.TASK_MODES} == _lib.TASK_MODES


class _Desc:
    """a valid descriptor with one term of every kind and one rule of every mode, and the ctypes arrays it points into"""

    def __init__(self):
        from nuclear_sim_amd.schema import SCHEMA
        self.lib = _lib
        level = SCHEMA.slot("pump.oil_level", 1)[1]
        count = SCHEMA.slot("maint.maintenance_actions_performed")[1]
        self.terms = (_lib.NpbTaskTerm * 16)()
        self.rules = (_lib.NpbTaskRule * 8)()
        for k, kind in enumerate(("value", "abs_err", "sq_err", "beyond", "excess", "bits", "delta")):
            T = self.terms[k]
            T.weight, T.kind = 0.5, _lib.TASK_KINDS[kind]
            if kind == "bits":
                T.column.kind, T.column.slot, T.mask = I32, count, 3
            elif kind == "sq_err":
                self.source(T.column, "f64")
                T.ref_from_column = 1
                T.ref_column.kind, T.ref_column.slot = F64, level
            else:
                T.column.kind, T.column.slot, T.direction, T.limit, T.ref = F64, level, -1, 40.0, 1.0
        self.source(self.rules[0].column, "u8")
        self.rules[0].mode, self.rules[0].mask = _lib.TASK_MODES["bits_any"], 0xFF
        self.rules[1].column.kind, self.rules[1].column.slot = F64, level
        self.rules[1].mode, self.rules[1].direction, self.rules[1].limit, self.rules[1].terminal_reward = _lib.TASK_MODES["beyond"], 1, 99.0, -5.0
        self.rules[2].column.kind, self.rules[2].column.slot, self.rules[2].mode = F64, level, _lib.TASK_MODES["nonfinite"]
        self.d = _lib.NpbTaskDesc()
        self.d.n_terms, self.d.terms, self.d.n_rules, self.d.rules, self.d.bias = 7, self.terms, 3, self.rules, 0.25
        self.d.reward, self.d.done, self.d.cause, self.d.terms_out = A8, A8 + 1, A8 + 4, A8 + 8

    def source(self, C, kind):
        C.from_source = 1
        C.source.base, C.source.type, C.source.rows, C.source.row_stride, C.source.plant_stride = A8, self.lib.SAMPLE_TYPES[kind], 1, 0, 1


def _why(D, n=70):
    return abi.why(abi.library().npb_task_check, ctypes.byref(D.d), n)


def test_the_check_accepts_a_valid_task_and_null():
    assert _why(_Desc()) is None
    assert abi.library().npb_task_check(None, 70) is None
    D = _Desc(); D.d.cause = None; D.d.terms_out = None       # both optional
    assert _why(D) is None
    D = _Desc(); D.d.n_terms = 0                               # rules alone
    assert _why(D) is None
    D = _Desc(); D.d.n_rules = 0                               # terms alone
    assert _why(D) is None
    D = _Desc(); D.terms[0].weight = float("inf")              # an infinite weight is the caller's business
    assert _why(D) is None


NAN = float("nan")


_set = abi.set_path


REFUSALS = [
    ("n_plants", None, "n_plants must be >= 1"),
    ("too many terms", _set(("d", "n_terms"), 17), "term count must be 0 .. NPB_TASK_TERMS_MAX (16)"),
    ("negative term count", _set(("d", "n_terms"), -1), "term count must be 0 .. NPB_TASK_TERMS_MAX (16)"),
    ("too many rules", _set(("d", "n_rules"), 9), "rule count must be 0 .. NPB_TASK_RULES_MAX (8)"),
    ("terms without their array", _set(("d", "terms"), None), "with their descriptors"),
    ("bad kind of member", _set(("terms", 0, "column", "kind"), 7), "bad field kind or slot"),
    ("bad slot", _set(("terms", 0, "column", "slot"), 1 << 20), "bad field kind or slot"),
    ("bad slot of a rule", _set(("rules", 1, "column", "slot"), -3), "bad field kind or slot"),
    ("bad slot of a ref column", _set(("terms", 2, "ref_column", "slot"), 1 << 20), "bad field kind or slot"),
    ("NULL base", _set(("terms", 2, "column", "source", "base"), None), "a side source has a NULL base"),
    ("unknown type", _set(("rules", 0, "column", "source", "type"), 9), "a side source has an unknown element type"),
    ("rows != 1", _set(("terms", 2, "column", "source", "rows"), 2), "a side source must have rows == 1"),
    ("unknown term kind", _set(("terms", 0, "kind"), 7), "an unknown term kind"),
    ("unknown rule mode", _set(("rules", 0, "mode"), 3), "an unknown rule mode"),
    ("BITS on a real column", _set(("terms", 5, "column", "kind"), F64), "NPB_TASK_BITS on a real-valued column"),
    ("BITS with mask 0", _set(("terms", 5, "mask"), 0), "NPB_TASK_BITS with mask 0"),
    ("BITS_ANY on a real source", _set(("rules", 0, "column", "source", "type"), 0), "NPB_TASK_RULE_BITS_ANY on a real-valued column"),
    ("BITS_ANY with mask 0", _set(("rules", 0, "mask"), 0), "NPB_TASK_RULE_BITS_ANY with mask 0"),
    ("term direction", _set(("terms", 3, "direction"), 0), "a BEYOND or EXCESS term with a direction outside {-1, +1}"),
    ("excess direction", _set(("terms", 4, "direction"), 2), "a BEYOND or EXCESS term with a direction outside {-1, +1}"),
    ("rule direction", _set(("rules", 1, "direction"), 0), "NPB_TASK_RULE_BEYOND with a direction outside {-1, +1}"),
    ("NaN weight", _set(("terms", 6, "weight"), NAN), "a NaN weight"),
    ("NaN term limit", _set(("terms", 4, "limit"), NAN), "a NaN limit"),
    ("NaN rule limit", _set(("rules", 1, "limit"), NAN), "a NaN limit"),
    ("NaN ref", _set(("terms", 1, "ref"), NAN), "a NaN ref"),
    ("NaN bias", _set(("d", "bias"), NAN), "a NaN bias"),
    ("NaN terminal reward", _set(("rules", 2, "terminal_reward"), NAN), "a NaN terminal reward"),
    ("NULL reward", _set(("d", "reward"), None), "a NULL output"),
    ("NULL done", _set(("d", "done"), None), "a NULL output"),
    ("misaligned reward", _set(("d", "reward"), A8 + 4), "a misaligned output"),
    ("misaligned terms", _set(("d", "terms_out"), A8 + 4), "a misaligned output"),
    ("misaligned cause", _set(("d", "cause"), A8 + 2), "a misaligned output"),
]


@pytest.mark.parametrize("what, change, reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_check_names_every_refusal(what, change, reason):
    abi.check_refusal(_Desc, _why, "npb_set_task: ", what, change, reason)


def test_the_check_refuses_a_task_with_neither_terms_nor_rules():
    D = _Desc()
    D.d.n_terms = D.d.n_rules = 0
    assert "neither reward terms nor termination rules" in _why(D)


def test_a_nan_ref_is_read_only_where_the_term_has_one():
    """ref belongs to ABS_ERR / SQ_ERR with a constant; limit and direction to BEYOND / EXCESS: elsewhere they are not looked at"""
    D = _Desc()
    D.terms[0].ref = NAN; D.terms[0].limit = NAN; D.terms[0].direction = 5      # a VALUE term
    D.terms[2].ref = NAN                                                        # SQ_ERR against a column
    assert _why(D) is None
