"""GPU: restarts from a start bank -- npb_set_start_bank / npb_set_start_slots / npb_restore_bank and the bank episode kernel that
npb_step runs for the autoreset while a bank and slots are set (include/npb.h).  A restore copies bank entry
((next_slot % M) + M) % M bit for bit and advances the slot; an episode started from the bank steps on as a fresh batch loaded with
those entries does; a scram or a time limit restarts from the bank with the finished episode's entry handed out; a bank of the
batch's own start states with identity slots is the snapshot path bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _env(n, **kw):
    from nuclear_sim_amd.env import BatchedPlantEnv
    return BatchedPlantEnv(n, **kw)


def _action_env(action, seeds, storage="f64"):
    """BatchedPlantEnv.action_test's batch with a choice of storage type"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    from nuclear_sim_amd import scenarios
    seeds = list(seeds)
    env = BatchedPlantEnv(len(seeds), dt=5.0, heat_source="constant", noise_enabled=True, noise_std_percent=0.1,
                          noise_seeds=[42] * len(seeds), maintenance=True, storage=storage)
    eff = float(env.get_field("pump.lubrication_effectiveness")[0].item())
    env.set_fields(scenarios.action_test_fields(action, seeds, eff, randomize=True))
    return env


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _np(t):
    return t.detach().cpu().numpy().copy()


def _same_np(a, b):
    a, b = np.ascontiguousarray(np.atleast_1d(a)), np.ascontiguousarray(np.atleast_1d(b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _poke_flow(env, plants):
    """drop the coolant flow of `plants` below the low-flow trip: they scram on the next step"""
    if len(plants):
        fl = env.get_field("prim.coolant_flow_rate").cpu().numpy()
        fl[list(plants)] = 4000.0
        env.set_field("prim.coolant_flow_rate", fl)


@pytest.mark.parametrize("storage,n,m", [("f64", 1000, 300), ("f64", 49152, 50000), ("f32", 1000, 300)])
def test_restore_from_bank_is_exact(storage, n, m):
    bank = _action_env("oil_top_off", range(m), storage)
    live = _action_env("oil_top_off", range(10 ** 6, 10 ** 6 + n), storage)
    from nuclear_sim_amd import _lib
    if n > 45056:
        assert _lib.load().npb_state_arena_segment(live._h) > 0 and _lib.load().npb_state_arena_segment(bank._h) > 0
    rng = np.random.default_rng(n + m)
    for t in range(3):
        live.step(power_setpoint=90.0, noise_z=rng.standard_normal(n))
    slots = rng.integers(-3 * m, 3 * m, n).astype(np.int32)          # any value: the entry is ((slot % M) + M) % M
    advance = 7
    live.set_start_bank(bank, slots=slots, advance=advance)
    fb, ib = bank.state_arrays()
    obs_b = bank.get_observation().clone()
    f1, i1 = live.state_arrays()
    mask = rng.random(n) < 0.4
    obs = live.restore_from_bank(mask).clone()
    f2, i2 = live.state_arrays()
    s = np.mod(slots.astype(np.int64), m)
    m_t = torch.as_tensor(mask, device=live.device)
    s_t = torch.as_tensor(s[mask], device=live.device)
    assert _same(f2[:, m_t], fb[:, s_t]) and _same(i2[:, m_t], ib[:, s_t]), "masked plants hold their bank entries"
    assert _same(f2[:, ~m_t], f1[:, ~m_t]) and _same(i2[:, ~m_t], i1[:, ~m_t]), "unmasked plants are unchanged"
    assert _same(obs[m_t], obs_b[s_t])
    nxt, start = _np(live.next_start_slots), _np(live.episode_start)
    assert np.array_equal(nxt[mask], (s[mask] + advance) % m) and np.array_equal(nxt[~mask], slots[~mask])
    assert np.array_equal(start[mask], s[mask]) and (start[~mask] == -1).all()
    live.close(); bank.close()


def _maint_slots():
    """(kind, slot) of every maint.* member"""
    from nuclear_sim_amd.schema import SCHEMA
    return [(k, s) for k, s, label, _ in SCHEMA.columns() if label.startswith("maint.")]


def test_truncation_from_the_bank_with_maintenance():
    """action_test(bank_seeds=...): every time limit restarts each plant from its next bank entry (p, p + n, ... mod M); the second
    episode steps as a fresh batch loaded with those entries does, maintenance events and counts included"""
    from nuclear_sim_amd.env import BatchedPlantEnv, INFO_COLUMNS
    from nuclear_sim_amd.schema import SCHEMA
    n, M, K = 256, 97, 30
    bank_seeds = range(5000, 5000 + M)
    A = BatchedPlantEnv.action_test("oil_top_off", range(n), autoreset=True, max_episode_steps=K, bank_seeds=bank_seeds)
    Bk = BatchedPlantEnv.action_test("oil_top_off", bank_seeds)
    fB, iB = Bk.state_arrays()
    count_slot = SCHEMA.slot("maint.maintenance_actions_performed")[1]
    counts_B = _np(iB[count_slot])
    rng = np.random.default_rng(11)
    lane = np.arange(n)
    restarts = 0
    entry = np.full(n, -1)
    zs = [rng.standard_normal(n) for _ in range(3 * K)]
    rec = {k: [] for k in ("obs", "rew", "done", "flags", "info", "counts", "final")}
    first_entry, mid = None, None
    for t in range(3 * K):
        o, r, d, info = A.step(power_setpoint=90.0, noise_z=zs[t])
        d_np, tr = _np(d).astype(bool), _np(info["truncated"]).astype(bool)
        assert np.array_equal(_np(info["episode_start"]), entry), t          # the entry of the episode this transition belonged to
        assert not d_np.any(), "no scram expected at 90 % power"
        assert np.array_equal(tr, np.full(n, t % K == K - 1)), t
        rec["obs"].append(_np(o)); rec["rew"].append(_np(r)); rec["done"].append(d_np); rec["flags"].append(_np(info["trip_flags"]))
        rec["info"].append(np.stack([_np(info[c]) for c in INFO_COLUMNS], 1)); rec["counts"].append(_np(info["maintenance_event_count"]))
        rec["final"].append(_np(info["final_observation"]))
        if tr.any():
            expect = (lane + restarts * n) % M
            restarts += 1
            entry = expect
            assert np.array_equal(_np(A.episode_start), expect), t
            assert np.array_equal(_np(A.next_start_slots), (expect + n) % M), t
            f, i = A.state_arrays()
            e_t = torch.as_tensor(expect, device=A.device)
            assert _same(f, fB[:, e_t]) and _same(i, iB[:, e_t]), "every reset plant holds its bank entry (step %d)" % t
            assert np.array_equal(rec["counts"][-1], counts_B[expect]), "the count column follows the restore"
            if first_entry is None:
                first_entry = expect
        if t == 2 * K - 2:      # the second episode's last state before its time limit restores it
            mid = A.state_arrays()
    assert restarts == 3
    R = {k: np.stack(v) for k, v in rec.items()}

    # the second episode (A's steps K .. 2K - 1) against a fresh batch loaded with the entries it started from
    C = BatchedPlantEnv.action_test("oil_top_off", range(n))
    e_t = torch.as_tensor(first_entry, device=C.device)
    C.load_state_arrays(fB[:, e_t], iB[:, e_t])
    assert _same_np(R["obs"][K - 1], _np(C.get_observation())), "the reset step returns the restored observation"
    fired = 0
    for k in range(K):
        t = K + k
        o, r, d, info = C.step(power_setpoint=90.0, noise_z=zs[t])
        o, r, d = _np(o), _np(r), _np(d).astype(bool)
        assert _same_np(R["rew"][t], r) and _same_np(R["done"][t], d) and _same_np(R["flags"][t], _np(info["trip_flags"])), k
        np.testing.assert_allclose(R["info"][t], np.stack([_np(info[c]) for c in INFO_COLUMNS], 1), rtol=1e-12, atol=0, err_msg=str(k))
        cc = _np(info["maintenance_event_count"])
        if k < K - 1:
            assert _same_np(R["obs"][t], o), k
            assert np.array_equal(R["counts"][t], cc), k
        else:       # A's time limit: the terminal observation went to final_observation
            assert _same_np(R["final"][t], o), k
            fired = int((cc - counts_B[first_entry]).max())
        if k == K - 2:
            fC, iC = C.state_arrays()
            for kind, slot in _maint_slots():
                a, c = (mid[0], fC) if kind == "f64" else (mid[1], iC)
                assert _same(a[slot], c[slot]), (kind, slot)
    assert fired >= 1, "no maintenance event fired after a bank restore"
    A.close(); Bk.close(); C.close()


@pytest.mark.parametrize("variant", [1, 5])
def test_scram_autoreset_from_the_bank(variant):
    """a scram restarts the plant from its bank entry on the same step: final_observation and info["episode_start"] describe the
    finished episode, obs and env.episode_start the new one"""
    from nuclear_sim_amd.env import equilibrium_state
    n, M, T, adv = 256, 50, 30, 3
    rng = np.random.default_rng(70 + variant)
    first = rng.integers(2, 12, n)
    second = np.where(rng.random(n) < 0.5, first + rng.integers(3, 10, n), T + 100)
    never = rng.random(n) < 0.1
    first[never] = T + 100; second[never] = T + 100
    acts = rng.choice([0, 1, 8, 8, 8], size=(T, n)).astype(np.int32)
    mags = rng.uniform(0.5, 1.5, (T, n))

    def make(autoreset):
        e = _env(n, heat_source="reactor", autoreset=autoreset)
        e.set_fields(equilibrium_state())
        e.set_step_kernel(variant)
        return e

    bank = _env(M, heat_source="reactor")      # the batch's start state but for one pump's oil level, which tells the entries apart
    bank.set_fields(equilibrium_state())
    oil_bank = rng.uniform(91.0, 99.0, M)
    bank.set_field("pump.oil_level", oil_bank, instance=1)
    obs_bank = _np(bank.get_observation())
    A, B = make(True), make(False)
    A.snapshot()
    slots = rng.integers(0, M, n).astype(np.int32)
    A.set_start_bank(bank, slots=slots, advance=adv)
    torch.cuda.synchronize()
    bank.close()
    e1 = slots % M
    e2 = (e1 + adv) % M
    started = np.full(n, -1)
    for t in range(T):
        _poke_flow(A, np.flatnonzero((first == t) | (second == t)))
        _poke_flow(B, np.flatnonzero(first == t))
        oa, ra, da, ia = A.step(action=acts[t], magnitude=mags[t])
        assert A.last_step_kernel() == {1: "npb_step_kernel", 5: "npb_step4_kernel"}[variant]
        oa, da, fin, es, ln = _np(oa), _np(da).astype(bool), _np(ia["final_observation"]), _np(ia["episode_start"]), _np(ia["episode_length"])
        ob, rb, db, ib = B.step(action=acts[t], magnitude=mags[t])
        ob, db = _np(ob), _np(db).astype(bool)
        assert np.array_equal(da, (first == t) | (second == t)), t
        assert np.array_equal(es, started), t           # the episode this transition belonged to
        for p in np.flatnonzero(da):
            if first[p] == t:
                assert _same_np(fin[p], ob[p]) and db[p], (p, t)      # terminal observation of the first episode, as B saw it
                assert ln[p] == t + 1
                assert _same_np(oa[p], obs_bank[e1[p]]), (p, t)       # the new episode's observation: bank entry e1
                started[p] = e1[p]
            else:
                assert ln[p] == t - first[p]
                assert _same_np(oa[p], obs_bank[e2[p]]), (p, t)
                started[p] = e2[p]
        assert np.array_equal(_np(A.episode_start), started), t
        if da.any():
            oil = _np(A.get_field("pump.oil_level", instance=1))
            assert np.array_equal(oil[da], oil_bank[started[da]]), t
        live = ~da & (t < first)
        assert _same_np(oa[live], ob[live]), t
    assert (started >= 0).sum() > n // 2
    A.close(); B.close()


def test_bank_of_the_start_states_is_the_snapshot_path():
    """set_start_bank(self) with identity slots and advance 0 restores every plant from its own start state: bit for bit the
    snapshot autoreset, at 65 536 plants with scrams and time limits on most steps"""
    from nuclear_sim_amd.env import equilibrium_state
    n, T, K = 65536, 240, 64
    rng = np.random.default_rng(65536)

    def make():
        e = _env(n, heat_source="reactor", autoreset=True, max_episode_steps=K)
        e.set_fields(equilibrium_state())
        e.set_field("pump.oil_level", np.random.default_rng(3).uniform(40.0, 100.0, n), instance=1)
        e.snapshot()
        return e

    A, B = make(), make()
    B.set_start_bank(B, slots=np.arange(n), advance=0)
    resets = 0
    for t in range(T):
        poke = np.flatnonzero(rng.random(n) < 0.01)
        _poke_flow(A, poke); _poke_flow(B, poke)
        sp = rng.uniform(80.0, 100.0, n)
        oa, ra, da, ia = A.step(power_setpoint=sp)
        oa, ra, da, ia = oa.clone(), ra.clone(), da.clone(), {k: v.clone() for k, v in ia.items()}
        ob, rb, db, ib = B.step(power_setpoint=sp)
        assert _same(oa, ob) and _same(ra, rb) and _same(da, db), t
        for k in ("trip_flags", "truncated", "episode_length", "episode_return", "final_observation"):
            assert _same(ia[k], ib[k]), (t, k)
        r = (db != 0) | (ib["truncated"] != 0)
        resets += int(r.sum().item())
        assert bool((B.episode_start[r] == torch.arange(n, device=B.device)[r]).all()), t
    assert resets > n
    fa, i_a = A.state_arrays()
    fb, i_b = B.state_arrays()
    assert _same(fa, fb) and _same(i_a, i_b)
    A.close(); B.close()


def test_refusals():
    from nuclear_sim_amd import _lib
    a, b = _env(64), _env(64, storage="f32")
    L, h = a.L, a._h
    with pytest.raises(_lib.NpbError, match="storage"):
        a.set_start_bank(b)
    with pytest.raises(_lib.NpbError, match="bank"):
        a.restore_from_bank()
    # a bank without slots is nothing to autoreset to; with slots it is, with no snapshot at all
    _lib.check(L.npb_set_start_bank(h, h, a._stream()), h)
    with pytest.raises(_lib.NpbError, match="snapshot"):
        _lib.check(L.npb_set_autoreset(h, 1, 0), h)
    with pytest.raises(ValueError):
        a.set_start_bank(a, advance=-1)
    col = torch.zeros(64, dtype=torch.int32, device=a.device)
    assert L.npb_set_start_slots(h, ctypes.c_void_p(col.data_ptr()), None, -1) == -1 and b"advance" in L.npb_last_error(h)
    assert L.npb_set_start_slots(h, None, None, 0) == -1
    a.set_start_bank(a)
    _lib.check(L.npb_set_autoreset(h, 1, 0), h)
    with pytest.raises(_lib.NpbError, match="snapshot"):
        a.set_start_bank(None)          # the autoreset restores from the bank and has nothing else
    with pytest.raises(_lib.NpbError, match="autoreset"):
        a.enable_diagnostics()
    _lib.check(L.npb_set_autoreset(h, 0, 0), h)
    a.enable_diagnostics()
    with pytest.raises(_lib.NpbError, match="diagnostics"):
        _lib.check(L.npb_set_autoreset(h, 1, 0), h)
    a.enable_diagnostics(False)
    a.set_start_bank(None)
    a.snapshot()
    _lib.check(L.npb_set_autoreset(h, 1, 0), h)
    a.set_start_bank(a)
    a.set_start_bank(None)              # the snapshot remains to fall back on
    a.close(); b.close()
