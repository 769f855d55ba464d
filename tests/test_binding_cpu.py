"""CPU: the boundary between the headers and the binding as a whole.  Every NPB_API prototype of include/npb.h has a row in
_lib.ENTRY_POINTS with as many parameters, each of the prototype's class, and the return type's restype, and the table names nothing the
headers do not declare (from the table and the header text alone: no library); every ctypes.Structure of _lib is laid out as a C compiler
lays out its npb_*_t (one compiled probe)."""
import ctypes
import inspect

import abi_support as abi
from nuclear_sim_amd import _lib

# nuclear_sim_amd/scenarios.py binds these of include/npb_seeds.h itself, where it calls them
BOUND_WHERE_USED = {"npb_seed_py_random", "npb_seed_np_random", "npb_seed_np_gauss", "npb_seed_set_threads"}
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "double": ctypes.c_double, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64,
           "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32}
# every ctypes.Structure of _lib and the C type it mirrors
STRUCTS = {
    "npb_params_t": _lib.NpbParams, "npb_maint_table_t": _lib.NpbMaintTable, "npb_component_maint_table_t": _lib.NpbComponentMaintTable,
    "npb_sample_source_t": _lib.NpbSampleSource, "npb_sampler_desc_t": _lib.NpbSamplerDesc,
    "npb_maint_summary_key_t": _lib.NpbMaintSummaryKey, "npb_maint_summary_desc_t": _lib.NpbMaintSummaryDesc,
    "npb_episode_streams_desc_t": _lib.NpbEpisodeStreamsDesc, "npb_episode_records_desc_t": _lib.NpbEpisodeRecordsDesc,
    "npb_column_stats_desc_t": _lib.NpbColumnStatsDesc, "npb_episode_record_stats_desc_t": _lib.NpbEpisodeRecordStatsDesc,
    "npb_event_trigger_t": _lib.NpbEventTrigger, "npb_event_windows_desc_t": _lib.NpbEventWindowsDesc,
    "npb_task_column_t": _lib.NpbTaskColumn, "npb_task_term_t": _lib.NpbTaskTerm, "npb_task_rule_t": _lib.NpbTaskRule, "npb_task_desc_t": _lib.NpbTaskDesc,
    "npb_feature_column_t": _lib.NpbFeatureColumn, "npb_features_desc_t": _lib.NpbFeaturesDesc,
    "npb_control_axis_t": _lib.NpbControlAxis, "npb_controls_desc_t": _lib.NpbControlsDesc,
    "npb_rollout_desc_t": _lib.NpbRolloutDesc, "npb_rollout_advantages_desc_t": _lib.NpbRolloutAdvantagesDesc,
    "npb_moments_desc_t": _lib.NpbMomentsDesc, "npb_minibatch_desc_t": _lib.NpbMinibatchDesc, "npb_normalizer_desc_t": _lib.NpbNormalizerDesc,
    "npb_policy_desc_t": _lib.NpbPolicyDesc, "npb_ppo_desc_t": _lib.NpbPpoDesc,
}


def _is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def _agrees(c_type, t):
    """a C parameter or return type against a ctypes type: any pointer with any pointer type -- a POINTER to one of STRUCTS only with its
    own C type --, a scalar with the ctypes type of its width and signedness"""
    words = c_type.replace("const ", "").split()
    if "*" in c_type:
        pointee = getattr(t, "_type_", None)
        return _is_pointer(t) and (pointee not in STRUCTS.values() or STRUCTS.get(words[0]) is pointee)
    return len(words) == 1 and SCALARS.get(words[0]) is t


def test_every_prototype_has_its_row_and_every_row_its_prototype():
    declared = abi.declared()
    rows = {}
    for _detect, functions in _lib.ENTRY_POINTS:
        for name, row in functions.items():
            assert name not in rows, "%s has two rows" % name
            rows[name] = row
    assert BOUND_WHERE_USED <= set(declared) and not BOUND_WHERE_USED & set(rows)
    assert set(rows) == set(declared) - BOUND_WHERE_USED, sorted(set(rows) ^ (set(declared) - BOUND_WHERE_USED))
    for detect, functions in _lib.ENTRY_POINTS:
        assert detect is None or detect in functions, detect
    for name, (restype, argtypes) in rows.items():
        ret, params = declared[name]
        assert len(argtypes or ()) == len(params), (name, params, argtypes)
        for c_type, t in zip(params, argtypes or ()):
            assert _agrees(c_type, t), (name, c_type, t)
        if ret in ("int", "void"):
            assert restype in (None, ctypes.c_int), (name, ret, restype)
        else:
            assert _agrees(ret, restype), (name, ret, restype)


def test_every_structure_of_the_binding_is_laid_out_as_the_compiler_lays_out_its_c_type():
    classes = [c for _n, c in inspect.getmembers(_lib, inspect.isclass) if issubclass(c, ctypes.Structure) and c.__module__ == _lib.__name__]
    assert len(classes) >= 28 and set(classes) == set(STRUCTS.values()), set(classes) ^ set(STRUCTS.values())
    got, _ = abi.probe(STRUCTS, rename={"input": "in"})
    want = abi.layout(STRUCTS)
    assert len(got) == len(want)
    k = 0
    for c_name, S in STRUCTS.items():      # per struct, so that a failure names it
        n = 1 + len(S._fields_)
        assert got[k:k + n] == want[k:k + n], (c_name, [f[0] for f in S._fields_], got[k:k + n], want[k:k + n])
        k += n
