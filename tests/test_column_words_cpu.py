"""CPU: a per-plant column is stated once.  The column statistics, the event windows and the task refuse a bad column with the same five
texts under their own prefix, wherever the column sits in the descriptor (npb_column_stats_check, npb_event_windows_check, npb_task_check:
no handle, no device memory read), and ``_lib.column_word`` is the answer all three requests give for every word of their vocabulary."""
import ctypes
import os
import subprocess

import pytest

from nuclear_sim_amd import _lib
from nuclear_sim_amd.env import INFO_COLUMNS
from nuclear_sim_amd.schema import SCHEMA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nuclear_sim_amd", "libnpb.so")
A8 = 0x10000      # an aligned address: the checks read no device memory
LEVEL = SCHEMA.slot("pump.oil_level", 1)[1]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nuclear_sim_amd", "csrc"), "-s"])
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the five refusals, three entry points
def _source(S):
    S.base, S.type, S.rows, S.row_stride, S.plant_stride = A8, _lib.SAMPLE_TYPES["f64"], 1, 0, 17
    return S


def _head(C, from_source):
    """the {from_source, kind, slot, source} head of a trigger or a task column: the member pump.oil_level[1], or a float64 source"""
    if from_source:
        C.from_source = 1
        _source(C.source)
    else:
        C.kind, C.slot = 0, LEVEL
    return C


class _Listed:
    """the one member and the one source of a descriptor that lists kinds[] / slots[] and sources[]"""

    def __init__(self, d):
        self.kinds, self.slots, self.side = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(LEVEL), (_lib.NpbSampleSource * 1)()
        _source(self.side[0])
        d.n_fields, d.kinds, d.slots, d.n_sources, d.sources = 1, self.kinds, self.slots, 1, self.side

    def bad_kind(self):
        self.kinds[0] = 7


def _column_stats():
    """(descriptor, {place: (what makes its member bad, its source)}, what keeps the arrays alive)"""
    d = _lib.NpbColumnStatsDesc()
    cols = _Listed(d)
    d.last, d.n_samples = A8, A8
    return d, {"column": (cols.bad_kind, cols.side[0])}, cols


def _event_windows():
    d = _lib.NpbEventWindowsDesc()
    cols = _Listed(d)
    trig = (_lib.NpbEventTrigger * 2)()
    for k in range(2):
        _head(trig[k], from_source=k)
        trig[k].mode, trig[k].direction, trig[k].limit = _lib.TRIGGER_MODES["beyond"], 1, 50.0
    d.n_triggers, d.triggers, d.pre, d.post, d.capacity = 2, trig, 1, 1, 8
    for name in _lib.EVENT_WINDOW_WORDS + ("fired", "time", "times", "values", "cursor"):
        setattr(d, name, A8)
    return d, {"recorded column": (cols.bad_kind, cols.side[0]),
               "trigger column": (lambda: setattr(trig[0], "kind", 7), trig[1].source)}, (cols, trig)


def _task():
    d = _lib.NpbTaskDesc()
    terms, rules = (_lib.NpbTaskTerm * 4)(), (_lib.NpbTaskRule * 2)()
    for k in range(4):      # a member and a source as the term's column; then as the ref_column of an abs_err term on a member
        _head(terms[k].column, from_source=k == 1)
        terms[k].weight = 1.0
        if k >= 2:
            terms[k].kind, terms[k].ref_from_column = _lib.TASK_KINDS["abs_err"], 1
            _head(terms[k].ref_column, from_source=k == 3)
    for k in range(2):
        _head(rules[k].column, from_source=k)
        rules[k].mode, rules[k].direction, rules[k].limit = _lib.TASK_MODES["beyond"], 1, 50.0
    d.n_terms, d.terms, d.n_rules, d.rules, d.reward, d.done = 4, terms, 2, rules, A8, A8
    return d, {"term column": (lambda: setattr(terms[0].column, "kind", 7), terms[1].column.source),
               "rule column": (lambda: setattr(rules[0].column, "kind", 7), rules[1].column.source),
               "ref_column": (lambda: setattr(terms[2].ref_column, "kind", 7), terms[3].ref_column.source)}, (terms, rules)


ENTRY_POINTS = {
    "npb_set_column_stats": (_column_stats, lambda L, d: L.npb_column_stats_check(ctypes.byref(d), 70)),
    "npb_set_event_windows": (_event_windows, lambda L, d: L.npb_event_windows_check(ctypes.byref(d), 70, 0)),
    "npb_set_task": (_task, lambda L, d: L.npb_task_check(ctypes.byref(d), 70)),
}
PLACES = [(who, place) for who, (make, _check) in ENTRY_POINTS.items() for place in make()[1]]
# fault -> (the text behind the prefix, what it does to the place's source; None = it spoils the member)
FAULTS = {
    "bad field kind or slot": (": bad field kind or slot", None),
    "NULL base": (": a side source has a NULL base", lambda S: setattr(S, "base", None)),
    "unknown element type": (": a side source has an unknown element type", lambda S: setattr(S, "type", 4)),
    "rows == 1": (": a side source must have rows == 1 (one value per plant)", lambda S: setattr(S, "rows", 2)),
    "plant stride >= 0": (": a side source needs a plant stride >= 0", lambda S: setattr(S, "plant_stride", -1)),
}


@pytest.mark.parametrize("who", list(ENTRY_POINTS))
def test_the_descriptors_below_are_good(L, who):
    make, check = ENTRY_POINTS[who]
    d, _places, _keep = make()
    assert check(L, d) is None


@pytest.mark.parametrize("fault", list(FAULTS))
@pytest.mark.parametrize("who,place", PLACES)
def test_each_column_fault_is_refused_with_one_text_under_the_callers_prefix(L, who, place, fault):
    make, check = ENTRY_POINTS[who]
    d, places, _keep = make()
    tail, spoil = FAULTS[fault]
    bad_member, source = places[place]
    if spoil is None:
        bad_member()
    else:
        spoil(source)
    why = check(L, d)
    assert why is not None, (who, place, fault)
    assert why.decode() == who + tail      # its own prefix, and the tail every other entry point and place gives


# ---------------------------------------------------------------------------------------------------------------- the words
ARRAY_MEMBER = next(name for name, (_sec, f) in SCHEMA.by_name.items() if f.count > 1)
COMMON = ["prim.sim_time", ("pump.oil_level", 1), ("sg.tube_wall_temp", 0), (ARRAY_MEMBER, 0, 1), "maint.maintenance_actions_performed",
          ("info", INFO_COLUMNS[0]), ("info", INFO_COLUMNS[-1]), ("obs", 0), ("obs", 5), "reward"]
TASK_ONLY = ["flags", "done", "maintenance", ("work_order", 0), ("completed", 1)]
KEYS = 2      # summary keys


def _stats_answer(word, task):
    req = _lib.column_stats_request([word], None, ("last",), INFO_COLUMNS, task)
    return {"member": req["members"][0], "side": None} if req["members"] else {"member": None, "side": req["sides"][0] + ("f64",)}


def _windows_answers(word, task):
    """the word as a recorded column, and as the column of a limit trigger"""
    req = _lib.event_windows_request([word], [(word, ">", 1.0)], 0, 0, INFO_COLUMNS, KEYS, task)
    recorded = {"member": req["members"][0], "side": None} if req["members"] else {"member": None, "side": req["sides"][0] + ("f64",)}
    return recorded, {k: req["triggers"][0][k] for k in ("member", "side")}


def _task_answer(word):
    return _lib.task_request([(word, 1.0)], (), 0.0, INFO_COLUMNS, KEYS)["columns"][0]


@pytest.mark.parametrize("task", [False, True])
@pytest.mark.parametrize("word", COMMON + ["task_reward"], ids=repr)
def test_the_resolver_is_the_answer_of_the_statistics_and_the_windows(word, task):
    if word == "task_reward" and not task:
        for ask in (lambda: _stats_answer(word, task), lambda: _windows_answers(word, task), lambda: _lib.column_word(word, INFO_COLUMNS, task)):
            with pytest.raises(ValueError, match="needs a task"):
                ask()
        return
    C = _lib.column_word(word, INFO_COLUMNS, task)
    assert (C["member"] is None) != (C["side"] is None)
    assert C["integer"] == (word == "maint.maintenance_actions_performed")
    want = {"member": C["member"], "side": C["side"]}
    assert _stats_answer(word, task) == want
    assert _windows_answers(word, task) == (want, want)


@pytest.mark.parametrize("word", COMMON + TASK_ONLY, ids=repr)
def test_the_resolver_is_the_answer_of_the_task(word):
    C = _lib.column_word(word, INFO_COLUMNS, integer_sides=True, summary_keys=KEYS)
    assert _task_answer(word) == C
    assert C["integer"] == (word in TASK_ONLY or word == "maint.maintenance_actions_performed")
    if word in COMMON:      # the shared words mean the same column in every vocabulary
        assert C == _lib.column_word(word, INFO_COLUMNS)


def test_the_answers_name_the_buffers_and_members_they_should():
    assert _lib.column_word(("obs", 5)) == {"member": None, "side": ("obs", 5, _lib.OBS_DIM, "f64"), "integer": False}
    assert _lib.column_word(("info", INFO_COLUMNS[2])) == {"member": None, "side": ("info", 2, len(INFO_COLUMNS), "f64"), "integer": False}
    assert _lib.column_word("reward")["side"] == ("reward", 0, 1, "f64")
    assert _lib.column_word("task_reward", task=True)["side"] == ("task_reward", 0, 1, "f64")
    assert _lib.column_word(("pump.oil_level", 1))["member"] == (0, LEVEL)
    count = (1, SCHEMA.slot("maint.maintenance_actions_performed")[1])
    words = dict(integer_sides=True, summary_keys=KEYS)
    assert _lib.column_word("maintenance", **words) == {"member": count, "side": None, "integer": True}
    assert _lib.column_word("flags", **words)["side"] == ("flags", 0, 1, "i32")
    assert _lib.column_word("done", **words)["side"] == ("done", 0, 1, "u8")
    assert _lib.column_word(("work_order", 1), **words)["side"] == ("n_created", 1, 1, "i32")
    assert _lib.column_word(("completed", 0), **words)["side"] == ("n_completed", 0, 1, "i32")


@pytest.mark.parametrize("word", TASK_ONLY, ids=repr)
@pytest.mark.parametrize("task", [False, True])
def test_the_tasks_words_are_no_columns_of_the_statistics_and_the_windows(word, task):
    """"flags" in the column statistics is the one that must never come in through a shared buffer list"""
    for ask in (lambda: _stats_answer(word, task), lambda: _windows_answers(word, task), lambda: _lib.column_word(word, INFO_COLUMNS, task)):
        with pytest.raises(ValueError, match="unknown column"):
            ask()
    assert _task_answer(word)["integer"]      # ... and the task admits it


def test_a_task_never_reads_its_own_reward():
    for ask in (lambda: _task_answer("task_reward"), lambda: _lib.column_word("task_reward", INFO_COLUMNS, integer_sides=True, summary_keys=KEYS)):
        with pytest.raises(ValueError, match="needs a task"):
            ask()
    assert _stats_answer("task_reward", True)["side"][0] == "task_reward"      # ... the statistics and the windows do, while one is set
    assert _windows_answers("task_reward", True)[0]["side"][0] == "task_reward"


@pytest.mark.parametrize("word", ["trip", "task", "no.such_member", ("obs", _lib.OBS_DIM), ("info", "no_such_column"), ("pump.oil_level", 99), 7],
                         ids=repr)
def test_a_word_of_no_vocabulary_is_refused_by_all(word):
    for ask in (lambda: _stats_answer(word, True), lambda: _windows_answers(word, True), lambda: _task_answer(word)):
        with pytest.raises((ValueError, TypeError)):
            ask()


def test_the_summary_key_and_the_mask_checks_keep_their_callers_word():
    with pytest.raises(ValueError, match=r"the 'work_order' trigger: the summary's keys are 0 \.\. 1, not 2"):
        _lib.event_windows_request(["reward"], [("work_order", 2)], 0, 0, INFO_COLUMNS, KEYS)
    with pytest.raises(ValueError, match=r"the 'work_order' column: the summary's keys are 0 \.\. 1, not 2"):
        _task_answer(("work_order", 2))
    with pytest.raises(ValueError, match="the 'completed' trigger reads the maintenance summary"):
        _lib.event_windows_request(["reward"], [("completed", 0)], 0, 0, INFO_COLUMNS, 0)
    with pytest.raises(ValueError, match="the 'completed' column reads the maintenance summary"):
        _lib.task_request([(("completed", 0), 1.0)], (), 0.0, INFO_COLUMNS, 0)
    with pytest.raises(ValueError, match=r"the \('trip', mask\) trigger needs 0 < mask < 2\*\*32, not 0"):
        _lib.event_windows_request(["reward"], [("trip", 0)], 0, 0, INFO_COLUMNS)
    with pytest.raises(ValueError, match=r"the \('task', mask\) trigger needs 0 < mask < 2\*\*32, not 4294967296"):
        _lib.event_windows_request(["reward"], [("task", 1 << 32)], 0, 0, INFO_COLUMNS, 0, True)
    with pytest.raises(ValueError, match=r"reward term 0 \('flags', 1\.0, 'bits', 0\): needs 0 < mask < 2\*\*32, not 0"):
        _lib.task_request([("flags", 1.0, "bits", 0)])


def test_the_order_of_the_task_triggers_refusals_is_kept():
    """no number, then no task, then out of range"""
    with pytest.raises((TypeError, ValueError), match="int"):
        _lib.event_windows_request(["reward"], [("task", "x")], 0, 0, INFO_COLUMNS)
    with pytest.raises(ValueError, match="needs a task"):
        _lib.event_windows_request(["reward"], [("task", 0)], 0, 0, INFO_COLUMNS)


def test_where_a_side_column_starts_in_its_buffer():
    """env.task_samples() -- the reference of the GPU tests -- and the binder share this rule, so it is pinned here: a summary table is
    [n_keys][n], every other buffer [n][width]"""
    from nuclear_sim_amd.env import BatchedPlantEnv

    class _Sized:
        n = 70
    assert BatchedPlantEnv._side_first(_Sized, "n_created", 2) == 140 and BatchedPlantEnv._side_first(_Sized, "n_completed", 1) == 70
    assert BatchedPlantEnv._side_first(_Sized, "info", 2) == 2 and BatchedPlantEnv._side_first(_Sized, "obs", 5) == 5
    assert BatchedPlantEnv._side_first(_Sized, "flags", 0) == 0
