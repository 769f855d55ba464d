"""GPU: caller-defined reward terms and termination rules formed on the device (npb_set_task, BatchedPlantEnv.set_task).

The reference is nuclear_sim_amd.task.evaluate, the numpy statement of a task, over the columns the task reads, read back behind every
step through the EXISTING field and buffer paths (env.task_samples: npb_get_field and the step's own output tensors).  Sums and products of
doubles, comparisons and copies: reward, done, cause and terms match by bits, with no tolerance anywhere.

The run: BatchedPlantEnv.action_test("oil_top_off", seeds=range(n), dt=5.0) with the automatic maintenance on, every plant with a setpoint
of its own, 70 plants (one full wave and a ragged one) or 130 (three waves), at most 48 steps.  Pokes before a step: a fuel temperature of
1500 (the plant scrams on that step), a pump oil level of 4 (the pump trips and stays tripped; the maintenance tops it off two steps later)
and an infinite ``mpump.last_violation_time`` of the spare pump's last parameter (a stamp the rule only compares: that parameter is never
scanned again and nothing else changes), which is what the NONFINITE rule reads.

The limits of BEYOND / EXCESS are not chosen beforehand: they are the median over the plants of that column at a middle step of a dry run
of a twin env WITHOUT a task (computed once and shared), so some plants are beyond them and some are not.  Every test asserts that what it
claims to cover fired on some plant and stayed quiet on another."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, N3, DT, STEPS, MID = 70, 130, 5.0, 24, 12
KERNEL_OF_VARIANT = {1: "npb_step_maint_kernel", 2: "npb_step2_wide_maint_kernel", 5: "npb_step4_maint_kernel"}
PUMP_TRIPS = 0xF00                                  # NPB_TRIP_FW_PUMP0 .. 3
STAMP = ("mpump.last_violation_time", 3, 15)        # the column of the NONFINITE rule
# before step t: {what: plants}; plants past the batch are left out
POKES = {3: {"fuel": [5, 100]}, 4: {"oil": [9, 64, 129]}, 5: {"stamp": [11, 69, 128]}, 9: {"fuel": [66]}}


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(t):
    return t.contiguous().view(torch.int64)


def _make(n=N, **kw):
    from nuclear_sim_amd.env import BatchedPlantEnv
    return BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, **kw)


def _setpoint(t, n):
    return 90.0 + 8.0 * np.sin(2.0 * np.pi * t / (20.0 + np.arange(n) % 7))


def _set(env, name, plants, value, instance=0, k=0):
    plants = [p for p in plants if p < env.n]
    if plants:
        v = _np(env.get_field(name, instance, k))
        v[plants] = value
        env.set_field(name, v, instance, k)


def _poke(env, t, pokes=POKES):
    for what, plants in pokes.get(t, {}).items():
        if what == "fuel":
            _set(env, "prim.fuel_temperature", plants, 1500.0)
        elif what == "oil":
            _set(env, "pump.oil_level", plants, 4.0, 0)
        else:
            _set(env, STAMP[0], plants, np.inf, STAMP[1], STAMP[2])


@functools.lru_cache(maxsize=None)
def _dry():
    """the twin WITHOUT a task, stepped and poked as the tests step and poke: per step the step's reward, done, trip flags and obs and the
    whole state (on the device), and the limits -- medians over the plants at step MID.  Computed once, never written"""
    env = _make()
    out = {"reward": [], "done": [], "flags": [], "obs": [], "f64": [], "i32": []}
    for t in range(STEPS):
        _poke(env, t)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, N))
        f, i = env.state_arrays()
        for name, x in (("reward", rew), ("done", done), ("flags", info["trip_flags"]), ("obs", obs), ("f64", f), ("i32", i)):
            out[name].append(x.clone())
        if t == MID:
            out["limits"] = {c: float(np.median(_np(env.get_field(*c)))) for c in (("pump.oil_level", 0), ("pump.oil_level", 1), ("sg.tube_wall_temp", 1))}
    env.close()
    return out


def _task(trip_rule=True):
    """8 or 9 terms -- every kind, members carried and output, info, obs, reward, integer sides -- and 3 or 4 rules, every mode"""
    lim = _dry()["limits"]
    terms = [("reward", 1.0),
             (("info", "electrical_power"), -0.001, "abs_err", 790.0),
             (("obs", 5), 0.5, "sq_err", ("obs", 6)),
             (("pump.oil_level", 0), -0.25, "beyond", "<", lim[("pump.oil_level", 0)]),
             (("sg.tube_wall_temp", 1), -0.01, "excess", ">", lim[("sg.tube_wall_temp", 1)]),
             (("pump.oil_level", 1), 0.125, "excess", "<", lim[("pump.oil_level", 1)]),
             ("flags", -3.0, "bits", PUMP_TRIPS),
             ("maintenance", -2.0, "delta"),
             (("pump.oil_level", 0), 1.5, "delta")]
    rules = [("done", -100.0), (("pump.oil_level", 1), "<", lim[("pump.oil_level", 1)], -7.0), (STAMP, "nonfinite", -0.5)]
    if trip_rule:
        rules.append(("trip", PUMP_TRIPS, -50.0))
    return dict(reward=terms, terminate=rules, bias=0.125)


class _Coverage:
    """which term kinds and rules fired on some plant and stayed quiet on another, over a run"""

    def __init__(self, spec):
        self.spec = spec
        self.fired = np.zeros(len(spec["terms"]), dtype=bool); self.quiet = self.fired.copy()
        self.r_fired = np.zeros(len(spec["rules"]), dtype=bool); self.r_quiet = self.r_fired.copy()

    def add(self, terms, cause):
        self.fired |= (terms != 0.0).any(axis=1); self.quiet |= (terms == 0.0).any(axis=1)
        for r in range(len(self.r_fired)):
            bit = (cause >> np.uint32(r)) & np.uint32(1)
            self.r_fired[r] |= bool(bit.any()); self.r_quiet[r] |= bool((bit == 0).any())

    def check(self):
        for t, T in enumerate(self.spec["terms"]):
            assert self.fired[t], "term %d (%s) was never non-zero" % (t, T["kind"])
            if T["kind"] in ("beyond", "excess", "bits", "delta"):
                assert self.quiet[t], "term %d (%s) was never zero" % (t, T["kind"])
        for r, R in enumerate(self.spec["rules"]):
            assert self.r_fired[r] and self.r_quiet[r], "rule %d (%s): fired %s, quiet %s" % (r, R["mode"], self.r_fired[r], self.r_quiet[r])


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("variant, storage, n", [(1, "f64", N), (2, "f64", N3), (5, "f64", N), (2, "f32", N3)])
def test_bit_for_bit_with_the_numpy_statement(variant, storage, n):
    """Per step the columns the task reads are read back and fed to task.evaluate; reward, done, cause and terms are its bits.  Fails
    without the feature: set_task does not exist"""
    from nuclear_sim_amd import task
    env = _make(n, storage=storage)
    env.set_step_kernel(variant)
    env.set_task(keep_terms=True, **_task())
    spec = env.task_spec()
    assert sorted({T["kind"] for T in spec["terms"]}) == sorted(task.KINDS) and sorted({R["mode"] for R in spec["rules"]}) == sorted(task.MODES)
    cover, prev, primed = _Coverage(spec), None, np.zeros(n, dtype=bool)
    for t in range(STEPS):
        _poke(env, t)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, n))
        w_rew, w_done, w_cause, w_terms, prev = task.evaluate(_np(env.task_samples()), prev, primed, spec)
        primed[:] = True
        g_rew, g_terms, g_cause = _np(rew), _np(info["task_terms"]), _np(info["task_cause"]).view(np.uint32)
        assert np.array_equal(g_rew.view(np.uint64), w_rew.view(np.uint64)), (t, np.nonzero(g_rew.view(np.uint64) != w_rew.view(np.uint64))[0][:4])
        assert np.array_equal(g_terms.view(np.uint64), w_terms.view(np.uint64)), (t, np.argwhere(g_terms.view(np.uint64) != w_terms.view(np.uint64))[:4])
        assert np.array_equal(_np(done), w_done) and np.array_equal(g_cause, w_cause), t
        assert np.all(np.isfinite(w_rew)), t          # (the infinite stamp reaches a rule only)
        cover.add(w_terms, w_cause)
    assert env.last_step_kernel() == KERNEL_OF_VARIANT[variant], env.last_step_kernel()
    cover.check()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def test_without_autoreset_the_task_only_adds_columns():
    """the step's own reward / done buffers, the trip flags, the obs and the whole state are those of the twin without a task, bit for
    bit, at every step; the rules are levels and keep reporting"""
    dry = _dry()
    env = _make()
    env.set_task(**_task())
    differs, level = False, np.zeros(N, dtype=np.int64)
    for t in range(STEPS):
        _poke(env, t)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, N))
        assert torch.equal(_bits(info["reference_reward"]), _bits(dry["reward"][t])), t
        assert torch.equal(info["scram_activated"], dry["done"][t]) and torch.equal(info["trip_flags"], dry["flags"][t]), t
        assert torch.equal(_bits(obs), _bits(dry["obs"][t])), t
        f, i = env.state_arrays()
        assert torch.equal(_bits(f), _bits(dry["f64"][t])) and torch.equal(i, dry["i32"][t]), t
        assert rew.data_ptr() != info["reference_reward"].data_ptr() and done.data_ptr() != info["scram_activated"].data_ptr()
        differs |= not torch.equal(_bits(rew), _bits(info["reference_reward"]))
        level += (_np(info["task_cause"]).view(np.uint32) & 4) != 0          # the NONFINITE rule
        assert torch.equal(done != 0, info["task_cause"] != 0), t
    assert differs
    assert level[11] == STEPS - 5 and level[69] == STEPS - 5 and level[10] == 0      # a level: every step from the poke on
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_autoreset_with_a_start_bank_ends_episodes_by_the_task():
    """max_episode_steps 7, restarts from a bank.  The plants restart on the step a rule fires; the carried return and the records' ret
    are the sequential sum of the task's rewards; terminated is the task's done; the record's cause is the terminal step's; the others
    are truncated; and a window armed before a termination that only the task sees (the NONFINITE rule) is captured early.
    The oil-level rule ends the episodes of about half the plants on every step, whatever the bank hands them, so the two plants of the
    window check are picked at step 10 among those whose episode began at step 7."""
    from nuclear_sim_amd import task
    L, steps, post = 7, 21, 4
    pokes = {3: {"fuel": [5]}, 16: {"fuel": [66]}}
    env = _make(autoreset=True, max_episode_steps=L, bank_seeds=range(100, 110))
    env.enable_episode_records()
    env.set_task(**_task(trip_rule=False))
    # armed by the plant clock passing 7.5 minutes -- the second step of every episode, due four steps later; the second trigger: the
    # NONFINITE rule's bit rising in the task's cause column
    env.enable_event_windows([("pump.oil_level", 0), "task_reward"], [("prim.sim_time", ">", 7.5), ("task", 4)], pre=2, post=post)
    rewards, length = [[] for _ in range(N)], np.zeros(N, dtype=np.int64)
    want, causes, picked = [], np.zeros(N, dtype=np.uint32), []
    for t in range(steps):
        _poke(env, t, pokes)
        if t == 10:
            picked = [p for p in range(N) if length[p] == 3][:2]
            assert len(picked) == 2
            _set(env, STAMP[0], picked, np.inf, STAMP[1], STAMP[2])
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, N))
        r, d, cause, trunc = _np(rew), _np(done), _np(info["task_cause"]).view(np.uint32), _np(info["truncated"])
        ret, ep_len, index = _np(info["episode_return"]), _np(info["episode_length"]), _np(info["episode_index"])
        assert np.array_equal(d != 0, cause != 0), t
        causes |= cause
        for p in range(N):
            rewards[p].append(r[p]); length[p] += 1
            assert ep_len[p] == length[p], (t, p)             # a plant a rule ended restarted on that very step: its next step counts from 1
            assert np.float64(task.episode_return(rewards[p])).view(np.uint64) == ret[p].view(np.uint64), (t, p)
            assert bool(trunc[p]) == (length[p] >= L and not d[p]), (t, p)            # truncation still applies where no rule fired
            if d[p] or trunc[p]:
                want.append((t, p, int(index[p]), int(length[p]), 1 if d[p] else 2, int(cause[p]), ret[p]))
                rewards[p], length[p] = [], 0
        if t == 10:      # ended by the task alone, and already a bank entry's start state: the stamp is gone
            assert np.all(cause[picked] & 4) and not _np(info["scram_activated"])[picked].any()
            assert np.all(np.isfinite(_np(env.get_field(*STAMP))[picked]))
        if t in pokes:
            assert np.all(cause[pokes[t]["fuel"]] & 1), t
    assert (causes & 1).any() and (causes & 2).any() and (causes & 4).any()          # each rule ended somebody's episode ...
    terminated, truncated = sum(w[4] == 1 for w in want), sum(w[4] == 2 for w in want)
    assert terminated >= 4 and truncated >= N // 4 and not (causes & 2).all()        # ... and left others alone
    rec = env.episode_records()
    assert len(rec["plant"]) == len(want) and rec["cause"].dtype == np.uint32
    want.sort(key=lambda w: (w[0], w[1]))
    for j, (t, p, index, ln, flags, cause, ret) in enumerate(want):
        assert (rec["step"][j], rec["plant"][j], rec["episode"][j], rec["length"][j], rec["flags"][j]) == (t, p, index, ln, flags), (j, t, p)
        assert rec["cause"][j] == cause, (j, t, p)
        assert rec["ret"][j].view(np.uint64) == np.float64(ret).view(np.uint64), (j, t, p)
        assert bool(rec["terminated"][j]) == (cause != 0) and bool(rec["truncated"][j]) == (cause == 0), (j, t, p)
    # the picked plants: armed at step 8 by the clock, due at 12; the task ends their episodes at 10: early, two samples short, and the
    # cause trigger found them armed
    win = env.event_windows()
    for p in picked:
        mine = [j for j in range(len(win["plant"])) if win["plant"][j] == p and win["step"][j] + win["n_post"][j] == 10]
        assert len(mine) == 1, (p, win["plant"].tolist(), win["step"].tolist())
        j = mine[0]
        assert bool(win["early"][j]) and win["trigger"][j] == 0 and (win["step"][j], win["n_pre"][j], win["n_post"][j]) == (8, 1, 2), (p, j)
        assert win["retriggers"][j] == 1 and np.isnan(win["values"][j, 2 + 3, 0]) and not np.isnan(win["values"][j, 2 + 2, 1])
    assert np.sum(~win["early"] & (win["n_post"] == post)) >= N // 4         # the undisturbed plants' windows ran their length
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_delta_terms_price_the_events_of_the_maintenance_log():
    """A DELTA term on the event count and one on a summary key's n_created row, weights 1: per step and plant they are the number of
    COMPLETED records and of oil_top_off CREATED records the log holds for that step -- and 0 on the first step after a restart"""
    from nuclear_sim_amd import _lib, maintlog
    L, steps = 20, 48
    pokes = {2: {"oil": [9, 64]}, 21: {"oil": [30]}, 25: {"fuel": [31]}}
    env = _make(autoreset=True, max_episode_steps=L, maintenance_log=16384)
    env.enable_maintenance_summary(["oil_top_off"])
    env.set_task(reward=[("maintenance", 1.0, "delta"), (("work_order", 0), 1.0, "delta")], terminate=[("done",)], keep_terms=True)
    top_off = _lib.maint_action_index("oil_top_off")
    first = np.ones(N, dtype=bool)                # the next step is the first of the plant's episode
    priced, unpriced, restarts = np.zeros(2), np.zeros(2), 0
    for t in range(steps):
        _poke(env, t, pokes)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, N))
        rec = env.maintenance_log_records(clear=True)
        completed = np.bincount(rec["plant"][rec["kind"] == maintlog.COMPLETED], minlength=N)
        created = np.bincount(rec["plant"][(rec["kind"] == maintlog.CREATED) & (rec["action"] == top_off)], minlength=N)
        events = np.stack([completed, created]).astype(np.float64)
        terms = _np(info["task_terms"])
        assert np.array_equal(terms, np.where(first, 0.0, events)), (t, np.argwhere(terms != np.where(first, 0.0, events))[:4])
        assert np.array_equal(_np(rew), terms[0] + terms[1])
        priced += np.where(first, 0.0, events).sum(axis=1); unpriced += np.where(first, events, 0.0).sum(axis=1)
        first = (_np(done) != 0) | (_np(info["truncated"]) != 0)
        restarts += int(first.sum())
    assert priced[0] >= 3 and priced[1] >= 3 and restarts >= 2 * N       # events were priced, in more than one episode of every plant
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_checkpoint_needs_the_task_state():
    """state_arrays() + task_state() at step 6, six more steps, both loaded again: the continuation is identical.  With the arena alone
    the first DELTA sample is taken against the wrong previous one, so task_state() matters"""
    steps, at = 12, 6
    z = np.random.default_rng(7).standard_normal((steps, N))
    env = _make()
    env.set_task(reward=[(("pump.oil_level", 0), 1.5, "delta"), ("maintenance", -2.0, "delta"), ("reward", 1.0)], terminate=[("done",)], keep_terms=True)

    def run(first, last):
        out = []
        for t in range(first, last):
            _poke(env, t)
            obs, rew, done, info = env.step(power_setpoint=_setpoint(t, N), noise_z=z[t])
            out.append(torch.cat([rew.view(1, N), info["task_terms"], done.to(torch.float64).view(1, N)]).clone())
        return torch.stack(out)
    run(0, at)
    f, i = env.state_arrays()
    state = env.task_state()
    assert state["prev"].shape == (2, N) and state["primed"].all() and np.array_equal(state["prev"][0], _np(env.get_field("pump.oil_level", 0)))
    a = run(at, steps)
    env.load_state_arrays(f, i)
    env.load_task_state(state)
    b = run(at, steps)
    assert torch.equal(_bits(a), _bits(b))
    env.load_state_arrays(f, i)                   # ... and without the task's own state
    c = run(at, steps)
    assert not torch.equal(_bits(a[0, 1]), _bits(c[0, 1]))                   # the first oil-level DELTA: against the sample of step 11
    assert torch.equal(_bits(a[0, 3]), _bits(c[0, 3])) and torch.equal(_bits(a[1:]), _bits(c[1:]))      # everything else is the arena's
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_lifecycle_of_a_task():
    from nuclear_sim_amd import _lib, task
    dry = _dry()
    env = _make()
    assert "reference_reward" not in env.step(power_setpoint=_setpoint(0, N))[3]
    env.set_task(**_task())
    env.enable_column_stats(["task_reward"], stats=("sum", "last"))
    env.enable_event_windows(["reward"], [("task", 4)], pre=1, post=1)
    series = []
    for t in range(1, 8):
        _poke(env, t)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, N))
        assert torch.equal(_bits(info["reference_reward"]), _bits(dry["reward"][t])) and set(info) >= {"task_cause", "reference_reward"}
        series.append(_np(rew))
    # the readers of the task's columns saw them: the folded sum is the sequential sum, the ("task", mask) trigger fired where the stamp went in
    cs = env.column_stats()
    assert np.array_equal(_np(cs["sum"][0]).view(np.uint64), np.array([task.episode_return(r) for r in np.array(series).T]).view(np.uint64))
    win = env.event_windows()
    assert sorted(win["plant"].tolist()) == [11, 69] and np.all(win["step"] == 4)      # (sample 0 of the windows is step 1)
    for what in ("column statistics", "event windows"):
        with pytest.raises(_lib.NpbError, match=what):
            env.set_task(None)
        with pytest.raises(_lib.NpbError, match=what):
            env.set_task(reward=[("reward", 2.0)])
        (env.enable_column_stats if what == "column statistics" else env.enable_event_windows)(None)
    env.set_task(None)
    for t in range(8, 10):          # the reference's columns again, from the next step on
        _poke(env, t)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, N))
        assert "reference_reward" not in info and "task_cause" not in info and done.data_ptr() == info["scram_activated"].data_ptr()
        assert torch.equal(_bits(rew), _bits(dry["reward"][t])) and torch.equal(done, dry["done"][t])
    with pytest.raises(ValueError, match="needs a task"):
        env.enable_column_stats(["task_reward"])
    with pytest.raises(_lib.NpbError, match="no task"):
        env.task_state()
    # the C ABI: a NULL output buffer is refused by the check, by name, before any device work -- and nothing is set
    d = _lib.NpbTaskDesc()
    rules = (_lib.NpbTaskRule * 1)()
    rules[0].column.from_source = 1
    rules[0].column.source.base, rules[0].column.source.type, rules[0].column.source.rows = env._done.data_ptr(), _lib.SAMPLE_TYPES["u8"], 1
    rules[0].column.source.plant_stride, rules[0].mode, rules[0].mask = 1, _lib.TASK_MODES["bits_any"], 0xFF
    out = torch.zeros(N, dtype=torch.float64, device=env.device)
    flag = torch.zeros(N, dtype=torch.uint8, device=env.device)
    d.n_rules, d.rules = 1, rules
    for reward_ptr, done_ptr in ((None, flag.data_ptr()), (out.data_ptr(), None)):
        d.reward, d.done = reward_ptr, done_ptr
        assert env.L.npb_set_task(env._h, ctypes.byref(d)) == -1
        assert b"a NULL output" in env.L.npb_last_error(env._h)
    for name in ("npb_task_clear", "npb_task_get_state"):
        args = (env._h, None, None) if name == "npb_task_clear" else (env._h, None, None, None, None)
        assert getattr(env.L, name)(*args) == -1 and b"no task set" in env.L.npb_last_error(env._h)
    cause = torch.zeros(64, dtype=torch.int32, device=env.device)
    assert env.L.npb_set_episode_record_task(env._h, ctypes.c_void_p(cause.data_ptr())) == -1 and b"no episode records" in env.L.npb_last_error(env._h)
    obs, rew, done, info = env.step(power_setpoint=_setpoint(10, N))
    assert torch.equal(_bits(rew), _bits(dry["reward"][10]))
    d.reward, d.done = out.data_ptr(), flag.data_ptr()           # and the same descriptor with its outputs is taken
    assert env.L.npb_set_task(env._h, ctypes.byref(d)) == 0
    assert env.L.npb_set_task(env._h, None) == 0
    env.close()


def test_the_cause_column_follows_the_records():
    """npb_set_episode_record_task by the rules of npb_set_episode_record_stats: records and a task both on; every successful
    npb_set_episode_records drops it (the env puts it back); while it is set the task cannot be replaced underneath it"""
    from nuclear_sim_amd import _lib
    env = _make(autoreset=True, max_episode_steps=3)
    env.enable_episode_records()
    env.step(power_setpoint=_setpoint(0, N))
    assert "cause" not in env.episode_records(clear=False)
    env.set_task(reward=[("reward", 1.0)], terminate=[("done",), (STAMP, "nonfinite")])
    assert env.L.npb_set_task(env._h, None) == -1 and b"npb_set_episode_record_task" in env.L.npb_last_error(env._h)
    _set(env, STAMP[0], [7], np.inf, STAMP[1], STAMP[2])
    for t in range(1, 3):
        env.step(power_setpoint=_setpoint(t, N))
    rec = env.episode_records()
    assert rec["cause"][rec["plant"] == 7].tolist() == [2] and rec["cause"].sum() == 2 and len(rec["plant"]) == N      # step 1: plant 7; step 2: the others, truncated
    env.enable_episode_records(capacity=256)      # new record columns: the cause column comes along
    _set(env, STAMP[0], [8], np.inf, STAMP[1], STAMP[2])
    env.step(power_setpoint=_setpoint(3, N))
    rec = env.episode_records()
    assert rec["plant"].tolist() == [8] and rec["cause"].tolist() == [2]
    env.set_task(None)                             # the env drops the column first
    env.step(power_setpoint=_setpoint(4, N))
    assert "cause" not in env.episode_records()
    env.close()


def test_the_cause_column_beside_the_records_statistics():
    """the records kernel takes both record-side descriptors through one device copy: the episode's statistics (of the task's reward
    too) and its cause word arrive together, and dropping either leaves the other"""
    from nuclear_sim_amd import _lib, task
    env = _make(autoreset=True, max_episode_steps=3)
    env.set_task(reward=[("reward", 0.5)], terminate=[("done",), (STAMP, "nonfinite", -1.0)])
    env.enable_column_stats(["task_reward", "reward"], stats=("sum",))
    env.enable_episode_records()
    series = []
    for t in range(3):
        if t == 1:
            _set(env, STAMP[0], [7], np.inf, STAMP[1], STAMP[2])
        series.append(_np(env.step(power_setpoint=_setpoint(t, N))[1]))
    rec = env.episode_records()
    assert rec["plant"].tolist() == [7] + [p for p in range(N) if p != 7] and rec["cause"].tolist() == [2] + [0] * (N - 1)
    assert np.array_equal(rec["stat_n_samples"], rec["length"]) and rec["length"].tolist() == [2] + [3] * (N - 1)
    want = [task.episode_return([s[p] for s in series[:ln]]) for p, ln in zip(rec["plant"], rec["length"])]
    assert np.array_equal(rec["stat_sum"][:, 0].view(np.uint64), np.array(want).view(np.uint64))      # the episode's summed task reward ...
    assert np.array_equal(rec["stat_sum"][:, 0].view(np.uint64), rec["ret"].view(np.uint64))         # ... which is its return
    assert env.L.npb_set_episode_record_stats(env._h, None) == 0          # the statistics leave, the cause word stays
    _set(env, STAMP[0], [8], np.inf, STAMP[1], STAMP[2])
    env.step(power_setpoint=_setpoint(3, N))
    assert env.L.npb_set_episode_record_task(env._h, None) == 0           # and the other way round: nothing left, the kernel takes no pointer
    _set(env, STAMP[0], [9], np.inf, STAMP[1], STAMP[2])
    env.step(power_setpoint=_setpoint(4, N))
    cause = _np(env._erec["dev"]["cause"])
    cursor = int(_np(env._erec["cursor"])[0])
    plants = _np(env._erec["dev"]["plant"])[:cursor]
    assert cursor >= 2 and plants[0] == 8 and cause[0] == 2               # step 3: plant 8, recorded with its cause
    assert 9 in plants.tolist() and cause[plants.tolist().index(9)] == 0  # step 4: plant 9 ended by the task, its cause no longer copied
    env.close()
