"""CPU: the numpy statement of a task (nuclear_sim_amd.task.evaluate) on hand-made columns -- every term kind, every rule mode, NaN
handling, DELTA unprimed behind an episode-index change, terminal rewards in rule order, the sequential rounding -- and the pure host
function that turns the caller's words into the request (nuclear_sim_amd._lib.task_request), which refuses each bad word by name."""
import numpy as np
import pytest

from nuclear_sim_amd import _lib, task

NAN, INF = float("nan"), float("inf")


def _term(col, weight, kind="value", **kw):
    return dict({"col": col, "weight": weight, "kind": kind, "ref": 0.0, "direction": 0, "limit": 0.0, "mask": 0}, **kw)


def _rule(col, mode, terminal_reward=0.0, **kw):
    return dict({"col": col, "mode": mode, "mask": 0, "direction": 0, "limit": 0.0, "terminal_reward": terminal_reward}, **kw)


def _eval(samples, terms=(), rules=(), bias=0.0, prev=None, primed=None):
    return task.evaluate(np.asarray(samples, dtype=np.float64), prev, primed, {"bias": bias, "terms": list(terms), "rules": list(rules)})


# ------------------------------------------------------------------------------------------------------------ the terms
def test_every_term_kind_on_hand_made_columns():
    v = [[2.0, -3.0, 5.0, 0.5],            # 0: a real column
         [1.0, 1.0, 7.0, 0.5],             # 1: a second one
         [0.0, 3.0, 4.0, -2147483648.0]]   # 2: an integer column, widened (the last: bit 31 alone, as an int32)
    terms = [_term(0, 2.0), _term(0, 1.0, "abs_err", ref=1.0), _term(0, 0.5, "sq_err", ref=("col", 1)),
             _term(0, -1.0, "beyond", direction=1, limit=2.0), _term(0, -1.0, "beyond", direction=-1, limit=2.0),
             _term(0, 3.0, "excess", direction=1, limit=1.0), _term(0, 3.0, "excess", direction=-1, limit=1.0),
             _term(2, 10.0, "bits", mask=0x80000002), _term(0, 1.0, "delta")]
    reward, done, cause, out, prev = _eval(v, terms, bias=100.0, prev=np.ones((9, 4)), primed=[True, True, False, True])
    want = np.array([[4.0, -6.0, 10.0, 1.0],             # value
                     [1.0, 4.0, 4.0, 0.5],               # |v - 1|
                     [0.5, 8.0, 2.0, 0.0],               # 0.5 (v - second)^2
                     [0.0, 0.0, -1.0, 0.0],              # v > 2: the limit itself is not beyond
                     [0.0, -1.0, 0.0, -1.0],             # v < 2
                     [3.0, 0.0, 12.0, 0.0],              # 3 (v - 1) above 1
                     [0.0, 12.0, 0.0, 1.5],              # 3 (1 - v) below 1
                     [0.0, 10.0, 0.0, 10.0],             # 3 & 2, and bit 31 of a negative int32
                     [1.0, -4.0, 0.0, -0.5]])            # v - 1; the unprimed plant gives 0
    assert np.array_equal(out, want)
    assert np.array_equal(reward, 100.0 + want.sum(axis=0))      # (small integers and halves: every order gives the same sum)
    assert not done.any() and not cause.any() and done.dtype == np.uint8 and cause.dtype == np.uint32
    assert np.array_equal(prev[8], v[0]) and np.array_equal(prev[:8], np.ones((8, 4)))      # only the delta row moves


def test_nan_samples():
    """a NaN sample gives a NaN reward through value, abs_err, sq_err and delta, whatever the weight; beyond and excess compare"""
    v = [[NAN, 1.0]]
    for kind, kw in (("value", {}), ("abs_err", {"ref": 0.0}), ("sq_err", {"ref": 0.0}), ("delta", {})):
        for w in (1.0, 0.0):
            reward, _, _, out, _ = _eval(v, [_term(0, w, kind, **kw)], bias=1.0, prev=np.zeros((1, 2)), primed=[True, True])
            assert np.isnan(reward[0]) and np.isnan(out[0, 0]) and not np.isnan(reward[1]), (kind, w)
    for kind in ("beyond", "excess"):
        for direction in (1, -1):
            reward, _, _, out, _ = _eval(v, [_term(0, 1.0, kind, direction=direction, limit=0.0)], bias=1.0)
            assert reward[0] == 1.0 and out[0, 0] == 0.0, (kind, direction)
    reward, _, _, _, _ = _eval([[1.0], [NAN]], [_term(0, 1.0, "abs_err", ref=("col", 1))])      # a NaN in the second column too
    assert np.isnan(reward[0])
    # an unprimed plant does not look at its (NaN) previous sample
    reward, _, _, _, prev = _eval([[3.0]], [_term(0, 1.0, "delta")], prev=[[NAN]], primed=[False])
    assert reward[0] == 0.0 and prev[0, 0] == 3.0


def test_delta_is_unprimed_after_an_episode_index_change():
    """the caller's loop as the device runs it: primed = the episode index is the one last seen; three plants, the second restarts at
    sample 2, the third is cleared by hand at sample 3"""
    series = np.array([[1.0, 10.0, 100.0], [2.0, 12.0, 103.0], [4.0, 0.0, 107.0], [7.0, 5.0, 112.0]])
    index = np.array([[0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 1, 0]])
    spec = {"bias": 0.0, "terms": [_term(0, 1.0, "delta")], "rules": []}
    prev, primed, seen, got = None, np.zeros(3, dtype=bool), index[0].copy(), []
    for s in range(4):
        primed &= index[s] == seen
        if s == 3:
            primed[2] = False
        seen = index[s].copy()
        reward, _, _, _, prev = task.evaluate(series[s:s + 1], prev, primed, spec)
        primed = np.ones(3, dtype=bool)
        got.append(reward)
    assert np.array_equal(got, [[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [2.0, 0.0, 4.0], [3.0, 5.0, 0.0]])


def test_the_sum_is_sequential_and_each_product_rounded_before_its_add():
    """bias + w0 f0 + w1 f1 in that order: 1 + 2^-53 stays 1 (ties to even), and stays 1 again; the reassociated sum 1 + (2^-53 + 2^-53)
    is the next double.  And a product is rounded on its own: 0.1 * 3 is not 0.3"""
    e = 2.0 ** -53
    reward, _, _, out, _ = _eval([[e], [e]], [_term(0, 1.0), _term(1, 1.0)], bias=1.0)
    assert reward[0] == 1.0 and 1.0 + (e + e) == np.nextafter(1.0, 2.0) and reward[0] != 1.0 + (out[0, 0] + out[1, 0])
    # the other order of the same three numbers differs in the last bit as well
    reward2, _, _, _, _ = _eval([[e], [1.0]], [_term(0, 1.0), _term(1, 1.0)], bias=e)
    assert reward2[0] == np.nextafter(1.0, 2.0)
    reward3, _, _, out3, _ = _eval([[3.0]], [_term(0, 0.1)], bias=-0.3)
    assert out3[0, 0] == 0.1 * 3.0 and reward3[0] == -0.3 + 0.1 * 3.0 and reward3[0] != 0.0


# ------------------------------------------------------------------------------------------------------------ the rules
def test_every_rule_mode_and_the_cause_word():
    v = [[0.0, 1.0, 4.0, 255.0, 256.0],          # an integer column
         [1.0, 2.0, 3.0, NAN, 2.0],              # a real column
         [1.0, INF, -INF, NAN, 1.7976931348623157e308]]
    rules = [_rule(0, "bits_any", mask=0xFF), _rule(1, "beyond", direction=1, limit=2.0), _rule(1, "beyond", direction=-1, limit=2.0),
             _rule(2, "nonfinite")]
    reward, done, cause, out, _ = _eval(v, rules=rules, bias=0.5)
    assert cause.tolist() == [0b0100, 0b1001, 0b1011, 0b1001, 0b0000]      # (a NaN is beyond nothing; DBL_MAX is finite)
    assert done.tolist() == [1, 1, 1, 1, 0] and out.shape == (0, 5) and np.array_equal(reward, np.full(5, 0.5))


def test_terminal_rewards_follow_the_terms_in_rule_order():
    """behind bias + w f come the terminal rewards of the rules that fired, one add each, first rule first: with 1, 2^-53, 2^-53 the order
    shows in the last bit"""
    e = 2.0 ** -53
    rules = [_rule(0, "beyond", e, direction=1, limit=0.0), _rule(0, "beyond", e, direction=1, limit=1.0), _rule(0, "beyond", -8.0, direction=1, limit=2.0)]
    reward, done, cause, _, _ = _eval([[0.0, 0.5, 1.5, 2.5]], [_term(0, 0.0)], rules, bias=1.0)
    assert cause.tolist() == [0, 1, 3, 7] and done.tolist() == [0, 1, 1, 1]
    assert reward.tolist() == [1.0, 1.0, 1.0, -7.0]            # (1 + e) + e == 1, not 1 + 2e; then - 8
    big = [_rule(0, "beyond", 1e308, direction=1, limit=0.0), _rule(0, "beyond", 1e308, direction=1, limit=0.0), _rule(0, "beyond", -1e308, direction=1, limit=0.0)]
    reward, _, _, _, _ = _eval([[1.0]], rules=big)
    assert reward[0] == INF                                     # (1e308 + 1e308) - 1e308 overflows; 1e308 + (1e308 - 1e308) would not


def test_evaluate_refuses_a_bad_spec():
    for spec, word in (({"terms": [], "rules": []}, "neither"), ({"terms": [_term(0, 1.0, "cube")]}, "unknown kind"),
                       ({"terms": [_term(0, NAN)]}, "weight is NaN"), ({"terms": [_term(0, 1.0, "bits", mask=0)]}, "mask"),
                       ({"terms": [_term(0, 1.0, "excess", direction=0, limit=1.0)]}, "direction"),
                       ({"terms": [_term(0, 1.0, "beyond", direction=1, limit=NAN)]}, "limit is NaN"),
                       ({"terms": [_term(0, 1.0, "abs_err", ref=NAN)]}, "ref is NaN"),
                       ({"rules": [_rule(0, "edge")]}, "unknown mode"), ({"rules": [_rule(0, "nonfinite", NAN)]}, "terminal reward is NaN"),
                       ({"terms": [_term(0, 1.0)] * 17}, "0 to 16"), ({"bias": NAN, "terms": [_term(0, 1.0)]}, "bias is NaN")):
        with pytest.raises(ValueError, match=word):
            task.evaluate(np.zeros((1, 2)), None, None, spec)


def test_episode_return_is_the_carried_sum():
    e = 2.0 ** -53
    assert task.episode_return([1.0, e, e]) == 1.0 and task.episode_return([e, e, 1.0]) == np.nextafter(1.0, 2.0) and task.episode_return([]) == 0.0


# ------------------------------------------------------------------------------------------------------------ the request
INFO = ("thermal_power", "electrical_power")


def _request(reward=(), terminate=(), bias=0.0, keys=0):
    return _lib.task_request(reward, terminate, bias, INFO, keys)


def test_task_request_turns_the_words_into_the_descriptor():
    req = _request([("reward", 1.0), (("info", "electrical_power"), -0.5, "abs_err", 900.0), (("obs", 5), 2.0, "sq_err", ("obs", 6)),
                    (("pump.oil_level", 1), -1.0, "beyond", "<", 40.0), (("pump.oil_level", 1), -0.25, "excess", ">", 99.0),
                    ("flags", -3.0, "bits", 0xF00), ("maintenance", -2.0, "delta"), (("work_order", 1), -4.0, "delta"), (("completed", 0), 1.0, "delta")],
                   [("done",), ("done", -100.0), ("trip", 8, -50), (("pump.oil_level", 1), "<", 10.0), ("reward", "nonfinite", -1.0), ("reward", "nonfinite")],
                   bias=0.125, keys=2)
    from nuclear_sim_amd.schema import SCHEMA
    cols = req["columns"]
    assert [T["kind"] for T in req["terms"]] == ["value", "abs_err", "sq_err", "beyond", "excess", "bits", "delta", "delta", "delta"]
    assert cols[req["terms"][0]["col"]] == {"member": None, "side": ("reward", 0, 1, "f64"), "integer": False}
    assert cols[req["terms"][1]["col"]]["side"] == ("info", 1, 2, "f64") and req["terms"][1]["ref"] == 900.0
    assert cols[req["terms"][2]["col"]]["side"][:2] == ("obs", 5) and req["terms"][2]["ref"] == ("col", req["terms"][2]["col"] + 1)
    assert cols[req["terms"][2]["ref"][1]]["side"][:2] == ("obs", 6)
    assert cols[req["terms"][3]["col"]]["member"] == (0, SCHEMA.slot("pump.oil_level", 1)[1]) and req["terms"][3]["col"] == req["terms"][4]["col"]      # one column, read once
    assert (req["terms"][3]["direction"], req["terms"][3]["limit"], req["terms"][4]["direction"], req["terms"][4]["limit"]) == (-1, 40.0, 1, 99.0)
    assert cols[req["terms"][5]["col"]] == {"member": None, "side": ("flags", 0, 1, "i32"), "integer": True} and req["terms"][5]["mask"] == 0xF00
    assert cols[req["terms"][6]["col"]] == {"member": (1, SCHEMA.slot("maint.maintenance_actions_performed")[1]), "side": None, "integer": True}
    assert cols[req["terms"][7]["col"]]["side"] == ("n_created", 1, 1, "i32") and cols[req["terms"][8]["col"]]["side"] == ("n_completed", 0, 1, "i32")
    rules = req["rules"]
    assert [(R["mode"], R["mask"], R["terminal_reward"]) for R in rules[:3]] == [("bits_any", 0xFF, 0.0), ("bits_any", 0xFF, -100.0), ("bits_any", 8, -50.0)]
    assert cols[rules[0]["col"]]["side"] == ("done", 0, 1, "u8") and rules[2]["col"] == req["terms"][5]["col"]
    assert (rules[3]["mode"], rules[3]["direction"], rules[3]["limit"], rules[3]["col"]) == ("beyond", -1, 10.0, req["terms"][3]["col"])
    assert (rules[4]["mode"], rules[4]["terminal_reward"], rules[5]["terminal_reward"], rules[4]["col"]) == ("nonfinite", -1.0, 0.0, req["terms"][0]["col"])
    assert req["bias"] == 0.125
    task.check({"bias": req["bias"], "terms": req["terms"], "rules": req["rules"]})      # the spec task.evaluate takes
    assert _request([], [("done",)])["terms"] == [] and _request([("reward", 1)], [])["rules"] == []


BAD_WORDS = [
    (dict(reward=[], terminate=[]), "needs a reward term or a termination rule"),
    (dict(reward=[("reward", 1.0)] * 17), "0 to 16 reward terms"),
    (dict(terminate=[("done",)] * 9), "0 to 8 termination rules"),
    (dict(reward=[("reward", 1.0)], bias=NAN), "bias is NaN"),
    (dict(reward=["reward"]), r"a term is \(column, weight\)"),
    (dict(reward=[("no.such_member", 1.0)]), "unknown column"),
    (dict(reward=[(("info", "nothing"), 1.0)]), "unknown info column"),
    (dict(reward=[(("obs", 22), 1.0)]), "unknown obs column"),
    (dict(reward=[(("pump.oil_level", 9), 1.0)]), "no such instance"),
    (dict(reward=[("reward", NAN)]), "the weight is NaN"),
    (dict(reward=[("reward", "heavy")]), "the weight must be a number"),
    (dict(reward=[("reward", 1.0, "cube")]), "unknown kind 'cube'"),
    (dict(reward=[("reward", 1.0, "value", 3.0)]), "takes nothing behind its kind"),
    (dict(reward=[("reward", 1.0, "abs_err")]), r"is \(column, weight, 'abs_err', ref\)"),
    (dict(reward=[("reward", 1.0, "sq_err", NAN)]), "the ref is NaN"),
    (dict(reward=[("reward", 1.0, "sq_err", "no.such_member")]), "unknown column"),
    (dict(reward=[("reward", 1.0, "beyond", ">=", 1.0)]), r"'>' \| '<', limit"),
    (dict(reward=[("reward", 1.0, "excess", ">", NAN)]), "the limit is NaN"),
    (dict(reward=[("reward", 1.0, "bits", 1)]), "needs an integer column"),
    (dict(reward=[("flags", 1.0, "bits", 0)]), r"0 < mask < 2\*\*32"),
    (dict(reward=[("flags", 1.0, "bits", 1 << 32)]), r"0 < mask < 2\*\*32"),
    (dict(reward=[(("work_order", 0), 1.0, "delta")]), "enable_maintenance_summary"),
    (dict(reward=[(("completed", 2), 1.0, "delta")], keys=2), r"keys are 0 \.\. 1"),
    (dict(reward=[(("work_order", "oil_top_off"), 1.0, "delta")], keys=2), "takes the index of a summary key"),
    (dict(terminate=[("scram",)]), "a rule is"),
    (dict(terminate=[("trip",)]), "a rule is"),
    (dict(terminate=[("trip", 0)]), r"0 < mask < 2\*\*32"),
    (dict(terminate=[("reward", ">", NAN)]), "the limit is NaN"),
    (dict(terminate=[("reward", "<", 1.0, NAN)]), "the terminal reward is NaN"),
    (dict(terminate=[("done", "big")]), "the terminal reward must be a number"),
    (dict(terminate=[("no.such_member", "nonfinite")]), "unknown column"),
    (dict(terminate=[("reward", ">", 1.0, -1.0, 5)]), "a rule is"),
]


@pytest.mark.parametrize("words, reason", BAD_WORDS, ids=[str(i) for i in range(len(BAD_WORDS))])
def test_task_request_refuses_each_bad_word_by_name(words, reason):
    with pytest.raises(ValueError, match=reason):
        _request(**words)


def test_the_readers_requests_know_the_task_columns_only_while_a_task_is_set():
    with pytest.raises(ValueError, match="needs a task"):
        _lib.column_stats_request(["task_reward"], info_columns=INFO)
    with pytest.raises(ValueError, match="needs a task"):
        _lib.event_windows_request(["reward"], [("task", 1)], 1, 1, INFO)
    req = _lib.column_stats_request(["task_reward", "reward"], info_columns=INFO, task=True)
    assert req["sides"] == [("task_reward", 0, 1), ("reward", 0, 1)]
    ew = _lib.event_windows_request(["task_reward"], [("task", 6), ("task_reward", "<", -5.0)], 2, 2, INFO, task=True)
    assert ew["triggers"][0]["side"] == ("task_cause", 0, 1, "i32") and ew["triggers"][0]["mode"] == "bits_rise" and ew["triggers"][0]["mask"] == 6
    assert ew["triggers"][1]["side"] == ("task_reward", 0, 1, "f64") and ew["numpy"] == [("bits", 6), ("<", -5.0)]
    with pytest.raises(ValueError, match=r"0 < mask < 2\*\*32"):
        _lib.event_windows_request(["reward"], [("task", 0)], 1, 1, INFO, task=True)
