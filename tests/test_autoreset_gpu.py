"""GPU: episodes -- npb_snapshot / npb_restore and the same-step autoreset with truncation that npb_step runs in its episode
kernel (include/npb.h, npb_set_autoreset).  Restores are bit-exact; an autoreset batch follows, bit for bit, a batch without
it up to each plant's terminal step and a fresh batch started from the snapshot after it; autoreset that never fires changes
nothing."""
import ctypes

import numpy as np
import pytest
import torch

from golden_util import RTOL, ATOL_SMALL

pytestmark = pytest.mark.gpu


def _env(n, **kw):
    from nuclear_sim_amd.env import BatchedPlantEnv
    return BatchedPlantEnv(n, **kw)


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _np(t):
    return t.detach().cpu().numpy().copy()


def _same_np(a, b):
    a, b = np.ascontiguousarray(np.atleast_1d(a)), np.ascontiguousarray(np.atleast_1d(b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("n", [1000, 49152])
def test_restore_is_exact(n, storage):
    from nuclear_sim_amd.env import equilibrium_state, config2_draws
    env = _env(n, heat_source="reactor", storage=storage)
    env.set_fields(equilibrium_state(*config2_draws(n)))
    rng = np.random.default_rng(n)
    env.set_field("pump.oil_level", rng.uniform(40.0, 100.0, n), instance=1)
    env.snapshot()
    f0, i0 = env.state_arrays()
    obs0 = env.get_observation().clone()
    for t in range(20):
        env.step(action=rng.choice([0, 1, 8, 8], n).astype(np.int32), magnitude=rng.uniform(0.5, 2.0, n))
    f1, i1 = env.state_arrays()
    mask = rng.random(n) < 0.3
    obs = env.restore(mask).clone()
    f2, i2 = env.state_arrays()
    m = torch.as_tensor(mask, device=env.device)
    assert not _same(f1[:, m], f0[:, m]), "20 steps must have moved the masked plants"
    assert _same(f2[:, m], f0[:, m]) and _same(i2[:, m], i0[:, m])
    assert _same(f2[:, ~m], f1[:, ~m]) and _same(i2[:, ~m], i1[:, ~m])
    assert _same(obs[m], obs0[m])


def test_restore_then_step_equals_a_fresh_start_with_maintenance():
    """restore(all) of the randomised oil_top_off plants (automatic maintenance on) steps on exactly as a new batch loaded with the
    snapshot's state does -- the maintenance cooldown cache and the event-count column follow the restore plant by plant, with no
    host-side invalidation -- and maintenance events fire after it."""
    from nuclear_sim_amd.env import BatchedPlantEnv
    from nuclear_sim_amd.schema import SCHEMA
    n, T0, T = 256, 30, 60
    a = BatchedPlantEnv.action_test("oil_top_off", seeds=range(n))
    a.snapshot()
    f0, i0 = a.state_arrays()
    counts0 = _np(i0[SCHEMA.slot("maint.maintenance_actions_performed")[1]])
    rng = np.random.default_rng(5)
    for t in range(T0):
        a.step(power_setpoint=90.0, noise_z=rng.standard_normal(n))
    a.restore()
    assert np.array_equal(_np(a._event_counts), counts0), "the event-count column follows the restore"

    b = BatchedPlantEnv.action_test("oil_top_off", seeds=range(n))
    b.load_state_arrays(f0, i0)
    assert _same(a.get_observation(), b.get_observation())
    fired = 0
    for t in range(T):
        z = rng.standard_normal(n)
        oa, ra, da, ia = a.step(power_setpoint=90.0, noise_z=z)
        oa, ra, ca = _np(oa), _np(ra), _np(ia["maintenance_event_count"])
        ob, rb, db, ib = b.step(power_setpoint=90.0, noise_z=z)
        assert _same_np(oa, _np(ob)) and _same_np(ra, _np(rb)), t
        assert np.array_equal(ca, _np(ib["maintenance_event_count"])), t
        fired = max(fired, int(ca.max()))
    fa, ia_ = a.state_arrays()
    fb, ib_ = b.state_arrays()
    assert _same(fa, fb) and _same(ia_, ib_)
    assert fired >= 1, "no maintenance event fired after the restore"


def _same_info(a, b, where):
    """info rows: bit for bit but for the last bits of sums -- the turbine's stage pass takes a wave-wide sequential path while any
    plant of the wave is off its fast path (npd_turbine.h), so a neighbour that is scrammed in one batch and running in the other
    can move the rounding of a plant's info columns (its state, obs, reward and flags stay bit-identical)"""
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, err_msg=str(where))


def _poke_flow(env, plants):
    """drop the coolant flow of `plants` below the low-flow trip: they scram on the next step"""
    if len(plants):
        fl = env.get_field("prim.coolant_flow_rate").cpu().numpy()
        fl[list(plants)] = 4000.0
        env.set_field("prim.coolant_flow_rate", fl)


@pytest.mark.parametrize("variant", [1, 5])
def test_autoreset_on_scram(oracle_lib, variant):
    from nuclear_sim_amd.env import equilibrium_state, INFO_COLUMNS
    n, T = 256, 40
    rng = np.random.default_rng(31 + variant)
    first = rng.integers(2, 20, n)                    # plant p scrams on step first[p] ...
    second = np.where(rng.random(n) < 0.4, first + rng.integers(3, 12, n), T + 100)   # ... and some on step second[p] again
    never = rng.random(n) < 0.1                       # and some never
    first[never] = T + 100; second[never] = T + 100
    acts = rng.choice([0, 1, 8, 8, 8], size=(T, n)).astype(np.int32)
    mags = rng.uniform(0.5, 1.5, (T, n))

    def make(autoreset):
        e = _env(n, heat_source="reactor", autoreset=autoreset)
        e.set_fields(equilibrium_state())
        e.set_step_kernel(variant)
        return e

    A, B = make(True), make(False)
    A.snapshot()
    fs, is_ = A.state_arrays()
    fs, is_ = _np(fs), _np(is_)
    rec = {k: [] for k in ("obs", "rew", "done", "flags", "info", "final", "len", "ret", "trunc")}
    recB = {k: [] for k in ("obs", "rew", "done", "flags", "info")}
    for t in range(T):
        _poke_flow(A, np.flatnonzero((first == t) | (second == t)))
        _poke_flow(B, np.flatnonzero(first == t))
        obs, rew, done, info = A.step(action=acts[t], magnitude=mags[t])
        assert A.last_step_kernel() == {1: "npb_step_kernel", 5: "npb_step4_kernel"}[variant]
        rec["obs"].append(_np(obs)); rec["rew"].append(_np(rew)); rec["done"].append(_np(done)); rec["flags"].append(_np(info["trip_flags"]))
        rec["info"].append(np.stack([_np(info[c]) for c in INFO_COLUMNS], 1)); rec["final"].append(_np(info["final_observation"]))
        rec["len"].append(_np(info["episode_length"])); rec["ret"].append(_np(info["episode_return"])); rec["trunc"].append(_np(info["truncated"]))
        obs, rew, done, info = B.step(action=acts[t], magnitude=mags[t])
        recB["obs"].append(_np(obs)); recB["rew"].append(_np(rew)); recB["done"].append(_np(done)); recB["flags"].append(_np(info["trip_flags"]))
        recB["info"].append(np.stack([_np(info[c]) for c in INFO_COLUMNS], 1))
    R = {k: np.stack(v) for k, v in rec.items()}
    RB = {k: np.stack(v) for k, v in recB.items()}
    assert not R["trunc"].any()
    expect_done = np.zeros((T, n), dtype=bool)
    for p in range(n):
        for s in (first[p], second[p]):
            if s < T:
                expect_done[s, p] = True
    assert np.array_equal(R["done"].astype(bool), expect_done), "every poke scrams its plant on that step, and only then"

    # ---- against B (no autoreset): identical up to and including each plant's first terminal step
    for p in range(n):
        s = min(first[p], T - 1)
        for k in ("rew", "done", "flags"):
            assert _same_np(R[k][: s + 1, p], RB[k][: s + 1, p]), (p, k)
        _same_info(R["info"][: s + 1, p], RB["info"][: s + 1, p], (p, "B"))
        if first[p] < T:
            assert _same_np(R["obs"][:s, p], RB["obs"][:s, p]), p
            assert _same_np(R["final"][s, p], RB["obs"][s, p]), p
            assert R["len"][s, p] == s + 1
            ret = 0.0
            for t in range(s + 1):
                ret += RB["rew"][t, p]
            assert _same_np(R["ret"][s, p], ret), p
        else:
            assert _same_np(R["obs"][:, p], RB["obs"][:, p]), p
            assert R["len"][T - 1, p] == T

    # ---- against C: a fresh batch loaded with the snapshot, plant p fed what A fed it after its first reset
    resets = first < T
    steps_c = T - 1 - int(first[resets].min())
    C = make(False)
    C.load_state_arrays(fs, is_)
    obs_c0 = _np(C.get_observation())
    assert _same_np(R["obs"][first[resets], np.flatnonzero(resets)], obs_c0[resets]), "the reset step returns the restored observation"
    recC = {k: [] for k in ("obs", "rew", "done", "flags", "info")}
    for k in range(steps_c):
        t = first + 1 + k                              # A's step that C's step k of plant p stands for
        live = resets & (t < T)
        tt = np.minimum(t, T - 1)
        a_k = np.where(live, acts[tt, np.arange(n)], 8).astype(np.int32)
        m_k = np.where(live, mags[tt, np.arange(n)], 1.0)
        _poke_flow(C, np.flatnonzero(live & (second == t)))
        obs, rew, done, info = C.step(action=a_k, magnitude=m_k)
        recC["obs"].append(_np(obs)); recC["rew"].append(_np(rew)); recC["done"].append(_np(done)); recC["flags"].append(_np(info["trip_flags"]))
        recC["info"].append(np.stack([_np(info[c]) for c in INFO_COLUMNS], 1))
    RC = {k: np.stack(v) for k, v in recC.items()}
    checked = 0
    for p in np.flatnonzero(resets):
        s1, s2 = first[p], second[p]
        end = min(s2, T - 1)
        ks = np.arange(end - s1)          # A's steps s1 + 1 .. end
        if len(ks) == 0:
            continue
        ta = s1 + 1 + ks
        for key in ("rew", "done", "flags"):
            assert _same_np(R[key][ta, p], RC[key][ks, p]), (p, key)
        _same_info(R["info"][ta, p], RC["info"][ks, p], (p, "C"))
        if s2 < T:
            assert _same_np(R["obs"][ta[:-1], p], RC["obs"][ks[:-1], p]), p
            assert _same_np(R["final"][s2, p], RC["obs"][ks[-1], p]), p
            assert R["len"][s2, p] == s2 - s1
            ret = 0.0
            for k in ks:
                ret += RC["rew"][k, p]
            assert _same_np(R["ret"][s2, p], ret), p
        else:
            assert _same_np(R["obs"][ta, p], RC["obs"][ks, p]), p
        checked += 1
    assert checked > n // 2

    # ---- against the CPU oracle on a sample: plant by plant, from the snapshot, with A's inputs after the first reset
    P = oracle_lib.Params(); P.heat_source = 1; P.dt = 1.0
    fA, iA = A.state_arrays()
    fA, iA = _np(fA), _np(iA)
    sample = rng.choice(np.flatnonzero(resets), 64, replace=False)
    for p in sample:
        ora = oracle_lib.OraclePlants(1, P)
        ora.set_state(fs[:, p], is_[:, p])
        o0 = ora.observe()[0]
        np.testing.assert_allclose(R["obs"][first[p], p], o0, rtol=RTOL, atol=1e-12)
        for t in range(first[p] + 1, T):
            if t == second[p]:
                ora.set("prim.coolant_flow_rate", 4000.0)
            o, r, d, fl, _ = ora.step(action=acts[t, p:p + 1], magnitude=mags[t, p:p + 1])
            assert int(d[0]) == int(R["done"][t, p]) and int(fl[0]) == int(R["flags"][t, p]), (p, t)
            np.testing.assert_allclose(R["rew"][t, p], r[0], rtol=RTOL, atol=1e-9, err_msg="plant %d step %d" % (p, t))
            if d[0]:
                np.testing.assert_allclose(R["final"][t, p], o[0], rtol=RTOL, atol=1e-12)
                ora.set_state(fs[:, p], is_[:, p])
                o = ora.observe()
            np.testing.assert_allclose(R["obs"][t, p], o[0], rtol=RTOL, atol=1e-12, err_msg="plant %d step %d" % (p, t))
        of, oi = ora.state(0)
        assert np.array_equal(iA[:, p], oi), p
        np.testing.assert_allclose(fA[:, p], of, rtol=RTOL, atol=ATOL_SMALL, err_msg="plant %d" % p)


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_truncation(storage):
    n, T, K = 128, 50, 7
    A = _env(n, storage=storage, autoreset=True, max_episode_steps=K)
    D = _env(n, storage=storage)
    obs_d0 = _np(D.get_observation())
    obs_d, final_d = [], None
    for t in range(K):
        o, r, d, info = D.step()
        obs_d.append(_np(o))
    rows = []
    for t in range(T):
        o, r, d, info = A.step()
        assert not _np(d).any()
        tr, ln = _np(info["truncated"]).astype(bool), _np(info["episode_length"])
        assert np.array_equal(tr, ln == K) and np.array_equal(ln, np.full(n, t % K + 1)), t
        if t % K == K - 1:
            assert _same_np(_np(info["final_observation"]), obs_d[K - 1]), t
            assert _same_np(_np(o), obs_d0), t
        else:
            assert _same_np(_np(o), obs_d[t % K]), t
        rows.append(_np(o))
    for t in range(K, T):
        assert _same_np(rows[t], rows[t - K]), t


def test_autoreset_that_never_fires_changes_nothing():
    n, T = 65536, 30
    rng = np.random.default_rng(65)
    A = _env(n, autoreset=True)
    B = _env(n)
    for t in range(T):
        sp = rng.uniform(80.0, 100.0, n)
        oa, ra, da, ia = A.step(power_setpoint=sp)
        assert A.last_step_kernel() == "npb_step4_kernel"
        oa, ra, da, ia = oa.clone(), ra.clone(), da.clone(), {k: v.clone() for k, v in ia.items()}
        ob, rb, db, ib = B.step(power_setpoint=sp)
        assert B.last_step_kernel() == "npb_step4_kernel"
        assert not bool(da.any())
        assert _same(oa, ob) and _same(ra, rb) and _same(da, db), t
        for k, v in ib.items():
            assert _same(ia[k], v), (t, k)
        assert not bool(ia["truncated"].any()) and bool((ia["episode_length"] == t + 1).all())
    fa, i_a = A.state_arrays()
    fb, i_b = B.state_arrays()
    assert _same(fa, fb) and _same(i_a, i_b)


def test_refusals():
    from nuclear_sim_amd import _lib
    env = _env(64)
    L, h = env.L, env._h
    with pytest.raises(_lib.NpbError, match="snapshot"):
        _lib.check(L.npb_set_autoreset(h, 1, 0), h)
    with pytest.raises(_lib.NpbError, match="snapshot"):
        env.restore()
    env.enable_diagnostics()
    env.snapshot()
    with pytest.raises(_lib.NpbError, match="diagnostics"):
        _lib.check(L.npb_set_autoreset(h, 1, 0), h)
    env.enable_diagnostics(False)
    _lib.check(L.npb_set_autoreset(h, 1, 0), h)
    with pytest.raises(_lib.NpbError, match="autoreset"):
        env.enable_diagnostics()
    obs = torch.zeros((64, 22), dtype=torch.float64, device=env.device)
    rc = L.npb_step(h, None, None, None, None, None, ctypes.c_void_p(obs.data_ptr()), None, None, None, None, env._stream())
    assert rc == -1 and b"done" in L.npb_last_error(h)
    env.close()
