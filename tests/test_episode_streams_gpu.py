"""GPU: episode streams (npb_set_episode_streams, BatchedPlantEnv(episode_streams=True)): each plant's heat-source noise and power
profile restart with its episode, on the device, in blocks the handle owns.

Expected values are numpy's (scenarios.episode_stream_rows, numpy.random.RandomState).  The noise rows are within the generator's
4 ulp of them (MAX_ULP_DRAW, tests/test_device_noise_gpu.py) and the integer generator state is numpy's exactly after the documented
number of calls per plant.  The profile's filter is held exact on the device's own draws: the mode reports no draws, so the rows are
compared bit for bit with those of a FRESH handle seeded with the same seed at the same row numbers (the mode off, npb_profile_fill),
whose reported draws scenarios.power_profile_rows turns into exactly those rows; against pure numpy the rows are within the 8 ulp of
tests/test_power_profile_gpu.py (MAX_ULP_ROW: draws 4 ulp off moved no row by more than 3)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_ULP_DRAW = 4
MAX_ULP_ROW = 8


def _ordered(a):
    i = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    mag = i & np.int64(0x7FFFFFFFFFFFFFFF)
    return np.where(i < 0, -mag, mag)


def _ulps(a, b):
    return np.abs(_ordered(a) - _ordered(b))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _np(t):
    return t.cpu().numpy().copy()


def _tbits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return torch.equal(_tbits(a), _tbits(b))


def _draws_after(rows, steps):
    """include/npb.h: the standard_normal() calls behind ``rows`` rows of a profile stream"""
    return rows + (1 if steps >= 3 and rows % steps >= 1 else 0)


def _numpy_state(seeds, calls):
    key = np.empty((len(seeds), 624), dtype=np.uint32)
    pos, has, cached = np.empty(len(seeds), dtype=np.int32), np.empty(len(seeds), dtype=np.int32), np.empty(len(seeds))
    for p, (s, c) in enumerate(zip(seeds, calls)):
        r = np.random.RandomState(int(s))
        if c:
            r.standard_normal(int(c))
        st = r.get_state()
        key[p], pos[p], has[p], cached[p] = st[1], st[2], st[3], st[4]
    return key, pos, has, cached


# ---- 1. the streams against numpy, under a script of restores --------------------------------------------------------------------
N, M, STEPS = 389, 5, 70          # two 256-lane blocks, seven waves, a ragged tail; block 64 runs out once (after step 63)
OWN_NOISE = 5000 + np.arange(N)
OWN_PROFILE = 42 + np.arange(N)
BANK_NOISE = np.array([7, 2 ** 32 - 1, 0, 99, 12345])
BANK_PROFILE = np.array([900001, 900002, 3, 900004, 2 ** 31])


def _masks():
    m = {k: np.zeros(N, dtype=bool) for k in "ABCDEF"}
    m["A"][7] = True                  # one lane of wave 0
    m["B"][64:128] = True             # every lane of wave 1
    m["C"][180:201] = True            # lanes straddling waves 2 and 3
    m["D"][N - 1] = True              # the last lane of the tail
    m["F"][300] = True                # (E: the empty mask)
    return m


def _script():
    """{step t: [(mask, from_bank), ...]}: the restores made after step t.  With block 5, t % 5 == 0 is a restart on the FIRST row of a
    block (one row taken, four pending), t % 5 == 4 on its LAST (nothing pending: the next refill begins the episode), t % 5 == 2 in
    between; with block 64, t = 63 is the last row and t = 64 the first.  Every kind of mask occurs at each; F the same plant on two
    consecutive steps."""
    m = _masks()
    script = {}
    for phase, start in enumerate((0, 4, 32)):           # first / last / mid of block 5 (32 % 5 == 2)
        for k, kind in enumerate("ABCDEF"):
            t = start + 5 * k
            script.setdefault(t, []).append((m[kind], (k + phase) % 2 == 0))
            if kind == "F":
                script.setdefault(t + 1, []).append((m[kind], (k + phase) % 2 == 1))
    union = m["A"] | m["B"] | m["C"] | m["D"] | m["F"]
    script.setdefault(63, []).append((union, True))      # block 64's last row
    script.setdefault(64, []).append((m["E"], False))    # ... and its first: the empty mask, then every kind at once, F again
    script[64].append((union, False))
    return script


def _model(T):
    """numpy's side of the script: per plant the restarts (step, noise seed, profile seed, bank entry or -1), then the expected rows"""
    from nuclear_sim_amd.scenarios import episode_stream_rows
    next_slot = np.arange(N) % M
    restarts = [[(0, int(OWN_NOISE[p]), int(OWN_PROFILE[p]), -1)] for p in range(N)]
    for t, calls in sorted(_script().items()):
        for mask, from_bank in calls:
            for p in np.flatnonzero(mask):
                if from_bank:
                    s = int(next_slot[p]); next_slot[p] = (s + N) % M
                    restarts[p].append((t + 1, int(BANK_NOISE[s]), int(BANK_PROFILE[s]), s))
                else:
                    restarts[p].append((t + 1, int(OWN_NOISE[p]), int(OWN_PROFILE[p]), -1))
    rows = episode_stream_rows([[r[:3] for r in plant] for plant in restarts], STEPS, T)
    return restarts, rows


@pytest.fixture(scope="module")
def fresh_rows():
    """per T: the mode-off rows of fresh handles -- every plant's own seeds (the twin that never restarts) and the bank's seeds -- with
    the filter checked on their reported draws, once"""
    from nuclear_sim_amd.env import BatchedPlantEnv, DeviceHeatSourceNoise, PowerProfile
    from nuclear_sim_amd.scenarios import power_profile_rows
    own_env, bank_env = BatchedPlantEnv(N), BatchedPlantEnv(M)
    noise = DeviceHeatSourceNoise(own_env, OWN_NOISE, block=STEPS)
    out = {"noise": np.stack([_np(noise.next()) for _ in range(STEPS)])}
    for T in (1, 2, 3, 7):
        R = (STEPS // T) * T              # whole profiles: power_profile_rows smooths a whole one
        for name, env, seeds in (("own", own_env, OWN_PROFILE), ("bank", bank_env, BANK_PROFILE)):
            sp, tg, z = (_np(x) for x in PowerProfile(env, seeds, T, block=STEPS).fill(STEPS, with_draws=True))
            for lo in range(0, R, T):
                want_tg, want_sp = power_profile_rows(z[lo:lo + T])
                assert np.array_equal(_bits(tg[lo:lo + T]), _bits(want_tg)) and np.array_equal(_bits(sp[lo:lo + T]), _bits(want_sp))
            out[(T, name)] = (sp, tg)
    own_env.close(); bank_env.close()
    return out


@pytest.mark.parametrize("T", [1, 2, 3, 7])
def test_streams_follow_numpy_under_scripted_restarts(T, fresh_rows):
    from nuclear_sim_amd.env import BatchedPlantEnv
    restarts, (want_noise, want_tg, want_sp) = _model(T)
    script = _script()
    # the rows of fresh handles at the same row numbers: plant p's rows since its last restart
    fresh_sp, fresh_tg = np.empty((STEPS, N)), np.empty((STEPS, N))
    never = np.array([len(r) == 1 for r in restarts])
    assert never.sum() > 100 and (~never).sum() > 80
    for p in range(N):
        for k, (lo, _, _, s) in enumerate(restarts[p]):
            hi = restarts[p][k + 1][0] if k + 1 < len(restarts[p]) else STEPS
            sp, tg = fresh_rows[(T, "own" if s < 0 else "bank")]
            col = p if s < 0 else s
            fresh_sp[lo:hi, p], fresh_tg[lo:hi, p] = sp[:hi - lo, col], tg[:hi - lo, col]
    got = {}
    for block in (1, 5, 64):
        env = BatchedPlantEnv(N, noise_enabled=True, noise_seeds=OWN_NOISE, noise_generator="device", autoreset=True,
                              power_profile=dict(seeds=OWN_PROFILE, steps=T))
        bank = BatchedPlantEnv(M)
        env.set_start_bank(bank)
        torch.cuda.synchronize(); bank.close()
        env.enable_episode_streams(block=block, bank_noise_seeds=BANK_NOISE, bank_profile_seeds=BANK_PROFILE)
        noise, sp, tg = np.empty((STEPS, N)), np.empty((STEPS, N)), np.empty((STEPS, N))
        for t in range(STEPS):
            obs, rew, done, info = env.step()
            rows = env.stream_rows
            noise[t], sp[t], tg[t] = _np(rows["noise"]), _np(rows["setpoint"]), _np(rows["target"])
            assert _same(info["target_power"], rows["target"])
            assert not bool(done.any()) and not bool(info["truncated"].any())      # only the script restarts plants
            assert _ulps(noise[t], want_noise[t]).max() <= MAX_ULP_DRAW, (block, t)
            assert np.array_equal(_bits(tg[t]), _bits(fresh_tg[t])), (block, t, np.flatnonzero(_bits(tg[t]) != _bits(fresh_tg[t]))[:8])
            assert np.array_equal(_bits(sp[t]), _bits(fresh_sp[t])), (block, t, np.flatnonzero(_bits(sp[t]) != _bits(fresh_sp[t]))[:8])
            assert _ulps(tg[t], want_tg[t]).max() <= MAX_ULP_ROW and _ulps(sp[t], want_sp[t]).max() <= MAX_ULP_ROW, (block, t)
            # a plant that never restarts: the rows of the mode-off twin
            assert np.array_equal(_bits(noise[t, never]), _bits(fresh_rows["noise"][t, never])), (block, t)
            for mask, from_bank in script.get(t, []):
                (env.restore_from_bank if from_bank else env.restore)(mask)
        # a restarted plant's first setpoint is its first target: the ramp began afresh
        for p in np.flatnonzero(~never):
            for lo, _, _, _ in restarts[p][1:]:
                if lo < STEPS:
                    assert _bits(sp[lo, p]) == _bits(tg[lo, p]), (block, p, lo)
        # the last bank restore's entries, as the library reports them
        last_entry = np.array([max((r for r in plant if r[3] >= 0), key=lambda r: r[0], default=(0, 0, 0, -1))[3] for plant in restarts])
        assert np.array_equal(_np(env.episode_start), last_entry)
        # positions and generator state: rows made since the restart = rows taken since it + rows drawn ahead and not yet taken
        pending = block - ((STEPS - 1) % block + 1)
        made = np.array([STEPS - plant[-1][0] + pending for plant in restarts])
        position, rows_made = env.profile_positions()
        assert np.array_equal(rows_made, made) and np.array_equal(position, made % T), block
        key, pos, has, cached = env._noise.get_state()
        want = _numpy_state([plant[-1][1] for plant in restarts], made)
        assert np.array_equal(key, want[0]) and np.array_equal(pos, want[1]) and np.array_equal(has, want[2]), block
        assert _ulps(cached, want[3]).max() <= MAX_ULP_DRAW
        key, pos, has, cached, _carried, one_position = env._profile.get_state()
        assert one_position == -1
        want = _numpy_state([plant[-1][2] for plant in restarts], [_draws_after(m, T) for m in made])
        assert np.array_equal(key, want[0]) and np.array_equal(pos, want[1]) and np.array_equal(has, want[2]), block
        assert _ulps(cached, want[3]).max() <= MAX_ULP_DRAW
        got[block] = (noise, sp, tg)
        env.close()
    for block in (5, 64):
        for a, b in zip(got[block], got[1]):
            assert np.array_equal(_bits(a), _bits(b)), block
    print("episode streams, T %d: %d restarts of %d plants, noise max %d ulp of numpy, rows max %d ulp" % (
        T, sum(len(r) - 1 for r in restarts), int((~never).sum()), int(_ulps(got[1][0], want_noise).max()),
        int(max(_ulps(got[1][1], want_sp).max(), _ulps(got[1][2], want_tg).max()))))


# ---- 2. every episode is a run ---------------------------------------------------------------------------------------------------
def test_every_episode_is_the_run_of_a_fresh_env():
    """action_test with a bank, a profile and device noise: each (plant, episode) after the first is bit for bit the run of a fresh
    action_test of that bank entry's scenario seed.  The twins are the lanes of ONE fresh batch without autoreset, one lane per (plant,
    episode) -- results do not depend on the lane (tests/test_gpu_parity.py) -- poked where the episode was.
    Truncation after 9 steps with profiles of 7; three plants scram mid-profile (steps 4, 12 and 20), each followed by a nine-step episode.
    The scrams are made as tests/test_start_bank_gpu.py::test_scram_autoreset_from_the_bank makes them, by the coolant flow: at dt = 5
    minutes a poked fuel temperature is back under its limit before the step's scram check (its rate is clipped to 10 K/s)."""
    from nuclear_sim_amd.env import BatchedPlantEnv
    n, steps, T, L = 130, 30, 7, 9
    bank_seeds = [1000, 1001, 1002, 1003, 1004]
    kw = dict(dt=5.0, power_profile_steps=T, noise_generator="device")
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), autoreset=True, max_episode_steps=L, bank_seeds=bank_seeds, episode_streams=True, **kw)
    env.set_step_kernel(1)
    pokes = {4: 3, 12: 70, 20: 129}                # before step t: plant

    def poke(e, plants):      # below the low-flow trip: the plant scrams on the next step
        v = e.get_field("prim.coolant_flow_rate").cpu().numpy()
        v[list(plants)] = 4000.0
        e.set_field("prim.coolant_flow_rate", v)

    rec = {k: [] for k in ("obs", "final", "reward", "target", "start", "index", "done", "length", "truncated")}
    for t in range(steps):
        if t in pokes:
            poke(env, [pokes[t]])
        obs, rew, done, info = env.step()
        assert env.last_step_kernel() == "npb_step_maint_kernel"
        for k, v in (("obs", obs), ("final", info["final_observation"]), ("reward", rew), ("target", info["target_power"]),
                     ("start", info["episode_start"]), ("index", info["episode_index"]), ("done", done), ("length", info["episode_length"]),
                     ("truncated", info["truncated"])):
            rec[k].append(_np(v))
    rec = {k: np.stack(v) for k, v in rec.items()}
    for t, p in pokes.items():
        assert rec["done"][t, p] and rec["length"][t, p] < T, (t, p)      # the scram ended the episode mid-profile
    # the (plant, episode) pairs after the first: their steps, bank entry and the episode step a poke fell on
    pairs = []
    for p in range(n):
        for e in range(1, int(rec["index"][:, p].max()) + 1):
            at = np.flatnonzero(rec["index"][:, p] == e)
            s = int(rec["start"][at[0], p])
            assert s >= 0 and np.all(rec["start"][at, p] == s) and np.array_equal(at, np.arange(at[0], at[0] + at.size))
            poked = [t - at[0] for t, q in pokes.items() if q == p and at[0] <= t <= at[-1]]
            pairs.append((p, at, s, poked))
    assert any(at.size > T and (p, int(at[0])) in {(3, 5), (70, 13), (129, 21)} for p, at, _, _ in pairs)
    twin = BatchedPlantEnv.action_test("oil_top_off", [bank_seeds[s] for _, _, s, _ in pairs], **kw)
    twin.set_step_kernel(1)
    worst = 0
    for j in range(L):
        plants = [k for k, (_, _, _, poked) in enumerate(pairs) if j in poked]
        if plants:
            poke(twin, plants)
        obs, rew, done, info = twin.step()
        assert twin.last_step_kernel() == "npb_step_maint_kernel"
        obs, rew, tg, done = _np(obs), _np(rew), _np(info["target_power"]), _np(done)
        for k, (p, at, s, _) in enumerate(pairs):
            if j >= at.size:
                continue
            t = at[j]
            ended = bool(rec["done"][t, p]) or bool(rec["truncated"][t, p])
            got_obs = rec["final"][t, p] if ended else rec["obs"][t, p]      # a reset plant's obs row already is the next episode's
            assert np.array_equal(_bits(got_obs), _bits(obs[k])), (p, int(t), j, s)
            assert _bits(rec["reward"][t, p]) == _bits(rew[k]) and _bits(rec["target"][t, p]) == _bits(tg[k]), (p, int(t), j, s)
            assert bool(rec["done"][t, p]) == bool(done[k])
            worst += 1
    print("every episode is a run: %d (plant, episode) pairs, %d steps compared bit for bit" % (len(pairs), worst))
    env.close(); twin.close()


# ---- 3. explicit columns win and consume nothing -------------------------------------------------------------------------------
def test_explicit_columns_consume_no_row():
    from nuclear_sim_amd.env import BatchedPlantEnv
    from nuclear_sim_amd.scenarios import episode_stream_rows
    n, T, block, steps = 130, 3, 4, 14
    noise_seeds, profile_seeds = 10 + np.arange(n), 500 + np.arange(n)
    env = BatchedPlantEnv(n, noise_enabled=True, noise_seeds=noise_seeds, noise_generator="device", autoreset=True,
                          power_profile=dict(seeds=profile_seeds, steps=T), episode_streams=False)
    env.enable_episode_streams(block=block)
    mask = np.zeros(n, dtype=bool); mask[[0, 63, 64, n - 1]] = True
    # step 3: explicit setpoint right after a restart (made after step 2).  The profile's rows 0..2 are taken by steps 0..2 and row 3,
    # the LAST of its block, by step 4 -- after the explicit step 3; the noise's last row of its second block (its row 7) is taken by
    # step 9, after the explicit noise of step 8 (steps 0..7 but 6 take noise rows 0..6; 6 is explicit too, in mid-block).
    explicit_sp, explicit_z = {3, 11}, {6, 8}
    takes_p = np.array([t not in explicit_sp for t in range(steps)]); takes_n = np.array([t not in explicit_z for t in range(steps)])
    restarts = [[(0, int(noise_seeds[p]), int(profile_seeds[p]))] + ([(3, int(noise_seeds[p]), int(profile_seeds[p]))] if mask[p] else []) for p in range(n)]
    want_noise, want_tg, want_sp = episode_stream_rows(restarts, steps, T, takes_noise=takes_n, takes_profile=takes_p)
    column = torch.full((n,), 93.0, dtype=torch.float64, device=env.device)
    zero = torch.zeros(n, dtype=torch.float64, device=env.device)
    for t in range(steps):
        before = {k: v.clone() for k, v in env.stream_rows.items()}
        obs, rew, done, info = env.step(power_setpoint=column if t in explicit_sp else None, noise_z=zero if t in explicit_z else None)
        rows = env.stream_rows
        if t in explicit_sp:
            assert "target_power" not in info and _same(rows["setpoint"], before["setpoint"]) and _same(rows["target"], before["target"])
        else:
            assert _ulps(_np(rows["target"]), want_tg[t]).max() <= MAX_ULP_ROW and _ulps(_np(rows["setpoint"]), want_sp[t]).max() <= MAX_ULP_ROW, t
        if t in explicit_z:
            assert _same(rows["noise"], before["noise"])
        else:
            assert _ulps(_np(rows["noise"]), want_noise[t]).max() <= MAX_ULP_DRAW, t
        if t == 4:      # the restarted plants' first row of the new episode: the ramp begins on the target
            assert np.array_equal(_bits(_np(rows["setpoint"])[mask]), _bits(_np(rows["target"])[mask]))
        if t == 2:
            env.restore(mask)
    # nothing was consumed by the explicit steps: the generators are numpy's after the rows made
    first = np.where(mask, 3, 0)
    for takes, explicit, which, lookahead in ((takes_n, explicit_z, env._noise, False), (takes_p, explicit_sp, env._profile, True)):
        taken = np.array([int(takes[f:].sum()) for f in first])
        since_fill = int(takes.sum()) % block              # rows taken of the block under way (every plant shares the cursor)
        made = taken + (block - since_fill if since_fill else 0)
        state = which.get_state()
        seeds = noise_seeds if which is env._noise else profile_seeds
        want = _numpy_state(seeds, [_draws_after(m, T) if lookahead else m for m in made])
        assert np.array_equal(state[0], want[0]) and np.array_equal(state[1], want[1]) and np.array_equal(state[2], want[2])
    env.close()


# ---- 4. off is off -------------------------------------------------------------------------------------------------------------------
def test_switched_off_is_the_env_without_the_mode():
    """the setup of tests/test_power_profile_gpu.py::test_the_profile_continues_across_an_autoreset: an env whose mode was switched on
    and off again before the first step gives the rows and states of one that never had it, bit for bit -- the streams run on across
    the autoreset"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    seeds, steps = list(range(300)), 20
    kw = dict(autoreset=True, max_episode_steps=steps, noise_generator="device", power_profile_steps=steps)
    plain = BatchedPlantEnv.action_test("oil_top_off", seeds, **kw)
    was_on = BatchedPlantEnv.action_test("oil_top_off", seeds, episode_streams=True, **kw)
    assert was_on.stream_rows is not None
    was_on.disable_episode_streams()
    assert was_on.stream_rows is None
    for t in range(45):
        (oa, ra, da, ia), (ob, rb, db, ib) = plain.step(), was_on.step()
        assert _same(oa, ob) and _same(ra, rb) and _same(da, db) and ia.keys() == ib.keys()
        for name in ia:
            assert _same(ia[name], ib[name]), (t, name)
        if t % steps == steps - 1:    # (every plant truncates here, and the one profile stream runs on into the next profile)
            assert bool(ia["truncated"].all())
    fa, ia_ = plain.state_arrays()
    fb, ib_ = was_on.state_arrays()
    assert _same(fa, fb) and _same(ia_, ib_)
    for a, b in zip(plain._profile.get_state(), was_on._profile.get_state()):
        assert np.array_equal(a, b)
    plain.close(); was_on.close()


# ---- 5. refusals on the device ----------------------------------------------------------------------------------------------------
def test_refusals_while_the_mode_is_on():
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv, DeviceHeatSourceNoise, PowerProfile
    n = 70
    seeds = np.arange(n, dtype=np.int64)
    env = BatchedPlantEnv(n, noise_enabled=True, noise_seeds=seeds, noise_generator="device", autoreset=True, power_profile=dict(seeds=seeds, steps=5))
    L, h, st = env.L, env._h, env._stream()
    out = torch.empty((4, n), dtype=torch.float64, device=env.device)
    ptr, sp = ctypes.c_void_p(out.data_ptr()), seeds.ctypes.data_as(ctypes.c_void_p)

    def refused(rc, word):
        assert rc == -1 and word in L.npb_last_error(h).decode(), L.npb_last_error(h)

    pos = np.empty(n, dtype=np.int32)
    refused(L.npb_profile_get_positions(h, pos.ctypes.data_as(ctypes.c_void_p), None, st), "episode streams are off")
    desc, _keep = _lib.episode_streams_desc(4, [1, 2, 3])
    refused(L.npb_set_episode_streams(h, ctypes.byref(desc), st), "without a start bank")
    env.enable_episode_streams(block=4)
    noise_state, profile_state = env._noise.get_state(), env._profile.get_state()
    calls = {"npb_noise_fill": lambda: L.npb_noise_fill(h, 4, ptr, st),
             "npb_profile_fill": lambda: L.npb_profile_fill(h, 4, ptr, None, None, st),
             "npb_noise_seed": lambda: L.npb_noise_seed(h, sp, st),
             "npb_profile_seed": lambda: L.npb_profile_seed(h, sp, 5, None, 0, None, 0, st),
             "npb_noise_set_state": lambda: L.npb_noise_set_state(h, *(a.ctypes.data_as(ctypes.c_void_p) for a in noise_state), st),
             "npb_profile_set_state": lambda: L.npb_profile_set_state(h, *(a.ctypes.data_as(ctypes.c_void_p) for a in profile_state[:5]), 0, st)}
    for name, call in calls.items():
        refused(call(), name + ": episode streams are on")
    refused(L.npb_set_autoreset(h, 0, 0), "episode streams are on")
    for method in (env._noise.next, env._profile.next, lambda: env._profile.fill(3), lambda: env._noise.set_state(*noise_state),
                   lambda: env._profile.set_state(*profile_state)):
        with pytest.raises(_lib.NpbError, match="episode streams are on"):
            method()
    assert env._profile.get_state()[5] == -1
    env.step()
    position, rows_made = env.profile_positions()
    assert np.all(position == 4) and np.all(rows_made == 4)
    # tables need the bank's entry count, and the bank may not change under them
    bank = BatchedPlantEnv(3)
    env.set_start_bank(bank)
    desc, _keep = _lib.episode_streams_desc(4, [1, 2])
    refused(L.npb_set_episode_streams(h, ctypes.byref(desc), st), "entry count")
    assert env.stream_rows is not None and env.profile_positions()[1][0] == 4      # a refused request leaves the mode as it was
    env.enable_episode_streams(block=4, bank_noise_seeds=[1, 2, 3])
    other = BatchedPlantEnv(4)
    refused(L.npb_set_start_bank(h, other._h, st), "bank seed tables")
    refused(L.npb_set_start_bank(h, None, st), "bank seed tables")
    torch.cuda.synchronize(); bank.close(); other.close()
    # off: the entry points work again, from the plants' own seeds
    env.disable_episode_streams()
    for name, call in calls.items():
        assert call() == 0, (name, L.npb_last_error(h))
    fresh = BatchedPlantEnv(n)
    a = PowerProfile(env, seeds, 5).fill(12)
    b = PowerProfile(fresh, seeds, 5).fill(12)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    assert _same(DeviceHeatSourceNoise(env, seeds, block=9).next(), DeviceHeatSourceNoise(fresh, seeds, block=9).next())
    env.close(); fresh.close()
