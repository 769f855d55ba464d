"""GPU: the data-gen runner's power profile drawn on the device per plant (npb_profile_seed / npb_profile_fill / npb_profile_ramp /
npb_profile_get_state / npb_profile_set_state, PowerProfile, BatchedPlantEnv(power_profile=...)).

The filter is held exact independently of the device's log: scenarios.power_profile_rows fed the draws the device reports (z_out)
equals the device's targets and setpoints bit for bit, at every block size and across profile ends.  The draws are within the
generator's 4 ulp of numpy's and the generator state is numpy's exactly after the documented number of draws (include/npb.h: the rows
made, plus one look-ahead inside a profile of three or more steps).  Against the reference's own rows (tests/golden/power_profile) the
setpoints and targets are within 8 ulp: perturbing every draw by up to 4 ulp moved no setpoint by more than 3 ulp over 4 096 seeds x
600 steps, and every stage is a continuous clamp, so a flipped comparison cannot jump; 8 is that plus headroom."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "power_profile", "*.npz")))
MAX_ULP_DRAW = 4        # the generator's contract (tests/test_device_noise_gpu.py)
MAX_ULP_ROW = 8         # setpoint and target against the reference (the module docstring)


def _env(n, **kw):
    from nuclear_sim_amd.env import BatchedPlantEnv
    return BatchedPlantEnv(n, **kw)


def _ordered(a):
    i = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    mag = i & np.int64(0x7FFFFFFFFFFFFFFF)
    return np.where(i < 0, -mag, mag)


def _ulps(a, b):
    return np.abs(_ordered(a) - _ordered(b))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _rows(profile, rows, block):
    """at least ``rows`` rows in blocks of ``block``: (setpoint, target, z) as [made, n] arrays, and how many rows were made"""
    parts, made = [], 0
    while made < rows:
        parts.append(torch.stack(profile.fill(block, with_draws=True)).cpu().numpy())
        made += block
    out = np.concatenate(parts, axis=1)
    return out[0], out[1], out[2], made


def _restate(z, steps, base=90.0, std=2.0):
    """scenarios.power_profile_rows over consecutive profiles of ``steps`` rows; the last row of an unfinished profile is dropped (the
    restatement would leave it unsmoothed, the device has looked one draw ahead)"""
    from nuclear_sim_amd.scenarios import power_profile_rows
    tg, sp = [], []
    for lo in range(0, z.shape[0], steps):
        t, s = power_profile_rows(z[lo:lo + steps], base, std)
        keep = t.shape[0] if t.shape[0] == steps or steps < 3 else t.shape[0] - 1
        tg.append(t[:keep]); sp.append(s[:keep])
    return np.concatenate(tg), np.concatenate(sp)


def _draws_after(rows, steps):
    """include/npb.h: the standard_normal() calls behind ``rows`` rows"""
    return rows + (1 if steps >= 3 and rows % steps >= 1 else 0)


def _numpy_state(seeds, draws):
    z = np.empty((draws, len(seeds)))
    key = np.empty((len(seeds), 624), dtype=np.uint32)
    pos, has, cached = np.empty(len(seeds), dtype=np.int32), np.empty(len(seeds), dtype=np.int32), np.empty(len(seeds))
    for p, s in enumerate(seeds):
        r = np.random.RandomState(int(s))
        z[:, p] = r.standard_normal(draws)
        st = r.get_state()
        key[p], pos[p], has[p], cached[p] = st[1], st[2], st[3], st[4]
    return z, (key, pos, has, cached)


@pytest.mark.parametrize("n,steps", [(4102, 48), (389, 1), (389, 2), (389, 3)])
def test_rows_at_every_block_size_and_across_profile_ends(n, steps):
    from nuclear_sim_amd.env import PowerProfile
    seeds = ([42 + i for i in range(n - 6)] + [0, 2 ** 32 - 1, 42, 42, 7, 7])
    R = 200
    env = _env(n)
    got = {}
    for block in (1, 37, 256):
        g = PowerProfile(env, seeds, steps, block=block)
        sp, tg, z, made = _rows(g, R, block)
        got[block] = (sp[:R], tg[:R], z[:R])
        # the filter alone, on the device's own draws: exact
        want_tg, want_sp = _restate(z, steps)
        m = want_tg.shape[0]
        assert m >= made - 1
        assert np.array_equal(_bits(tg[:m]), _bits(want_tg)), block
        assert np.array_equal(_bits(sp[:m]), _bits(want_sp)), block
        # the generators: numpy's after the documented number of draws
        key, pos, has, cached, carried, position = g.get_state()
        assert position == made % steps
        want_z, state = _numpy_state(seeds, _draws_after(made, steps))
        assert np.array_equal(key, state[0]) and np.array_equal(pos, state[1]) and np.array_equal(has, state[2])
        assert _ulps(cached, state[3]).max() <= MAX_ULP_DRAW
        ulp = _ulps(z, want_z[:made])          # row t's draw is the stream's draw t: no profile skips or repeats one
        assert ulp.max() <= MAX_ULP_DRAW, block
    for block in (37, 256):
        for a, b in zip(got[block], got[1]):
            assert np.array_equal(_bits(a), _bits(b)), block
    print("profile rows, steps %d: %d draws, %.6f bit-identical to numpy, max %d ulp" % (steps, ulp.size, float(np.mean(ulp == 0)), int(ulp.max())))
    env.close()


def test_rows_against_the_reference_fixtures():
    """every fixture case as lanes of one batch (per-plant base / std columns; eleven copies of each, for a ragged batch of more than
    one block), every horizon, two runners in a row"""
    from nuclear_sim_amd.env import PowerProfile
    cases = [np.load(p) for p in GOLDEN]
    assert len(cases) >= 5
    seeds = np.concatenate([g["seeds"] for g in cases])
    base = np.concatenate([np.full(len(g["seeds"]), float(g["base_power_percent"])) for g in cases])
    std = np.concatenate([np.full(len(g["seeds"]), float(g["noise_std_percent"])) for g in cases])
    copies = 11
    seeds, base, std = np.tile(seeds, copies), np.tile(base, copies), np.tile(std, copies)
    env = _env(len(seeds))
    worst = {"setpoint": 0, "target": 0}
    same = total = 0
    for T in (int(T) for T in cases[0]["horizons"]):
        g = PowerProfile(env, seeds, T, base, std, block=64)
        sp, tg, _, _ = _rows(g, 2 * T, 2 * T)
        want_sp = np.tile(np.concatenate([c["setpoint_%d" % T].reshape(2 * T, -1) for c in cases], axis=1), (1, copies))
        want_tg = np.tile(np.concatenate([c["target_%d" % T].reshape(2 * T, -1) for c in cases], axis=1), (1, copies))
        u_sp, u_tg = _ulps(sp, want_sp), _ulps(tg, want_tg)
        worst["setpoint"] = max(worst["setpoint"], int(u_sp.max())); worst["target"] = max(worst["target"], int(u_tg.max()))
        same += int(np.sum(u_sp == 0)); total += u_sp.size
    print("device profile vs the reference's rows: max %d ulp (setpoint), %d ulp (target), %.4f of the setpoints bit-identical"
          % (worst["setpoint"], worst["target"], same / total))
    assert worst["setpoint"] <= MAX_ULP_ROW and worst["target"] <= MAX_ULP_ROW
    env.close()


def test_per_plant_load_profiles():
    from nuclear_sim_amd.env import PowerProfile
    n, steps = 701, 60
    base = np.array([90.0, 98.0, 104.9])[np.arange(n) % 3]
    std = np.array([2.0, 0.2, 2.0])[np.arange(n) % 3]
    seeds = 3 + np.arange(n) // 3                     # lane 2 is the fixture's clipped case: seed 3 at 104.9 / 2.0
    env = _env(n)
    g = PowerProfile(env, seeds, steps, base, std, block=50)
    sp, tg, z, made = _rows(g, 150, 50)
    want_tg, want_sp = _restate(z, steps, base, std)
    m = want_tg.shape[0]
    assert np.array_equal(_bits(tg[:m]), _bits(want_tg)) and np.array_equal(_bits(sp[:m]), _bits(want_sp))
    assert int(np.sum(104.9 + 0.2 * z[:60, 2] > 105.0)) == 17      # 17 of its 60 raw values are clipped
    assert tg[:, 2::3].max() <= 105.0 and abs(tg[:, 1::3].mean() - 98.0) < 0.1 and abs(tg[:, 0::3].mean() - 90.0) < 0.1
    c = np.load(os.path.join(ROOT, "tests", "golden", "power_profile", "clipped_104p9_2p0.npz"))
    j = list(c["seeds"]).index(3)
    assert _ulps(sp[:60, 2], c["setpoint_60"][0, :, j]).max() <= MAX_ULP_ROW
    # a scalar is every plant's value
    g = PowerProfile(env, seeds, steps, 98.0, 0.2, block=50)
    sp1, tg1, z1, _ = _rows(g, 60, 60)
    want_tg, want_sp = _restate(z1, steps, 98.0, 0.2)
    assert np.array_equal(_bits(tg1), _bits(want_tg)) and np.array_equal(_bits(sp1), _bits(want_sp))
    env.close()


def test_the_ramp_alone_follows_numpy_across_calls():
    from nuclear_sim_amd.scenarios import power_profile_ramp
    n, k = 333, 50
    rng = np.random.default_rng(11)
    steps = rng.choice([0.02, -0.02, 0.019999999, -0.03, 0.0, 0.04, 0.5, -0.5], size=(k, n))
    targets = np.cumsum(steps, axis=0)
    targets[:3, 0] = [0.0, 0.02, 0.04]          # differences of exactly 0.02: not above the rate, taken as they are
    targets[:, 1] = 90.0 + 0.02 * np.arange(k)
    targets[:, 2:] += rng.uniform(20.0, 105.0, n - 2)
    want, _ = power_profile_ramp(targets)
    assert np.any(np.abs(targets[1:] - want[:-1]) == 0.02) and np.any(np.abs(targets[1:] - want[:-1]) > 0.02)
    env = _env(n)
    t = torch.from_numpy(targets).to(env.device)
    a = env.ramp_setpoints(t[:17])
    b = env.ramp_setpoints(t[17:])
    got = torch.cat([a, b]).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    one = env.ramp_setpoints(t[0])              # one row: carried from the call before
    assert np.array_equal(_bits(one.cpu().numpy()), _bits(power_profile_ramp(targets[:1], want[-1])[0][0]))
    env.forget_ramp()
    again = env.ramp_setpoints(t).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(want))
    env.close()


def _tbits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return torch.equal(_tbits(a), _tbits(b))


def _same_step(ra, rb, target=None):
    obs_a, rew_a, done_a, info_a = ra
    obs_b, rew_b, done_b, info_b = rb
    assert _same(obs_a, obs_b) and _same(rew_a, rew_b) and _same(done_a, done_b)
    if target is None:
        assert "target_power" not in info_a
    else:
        assert _same(info_a["target_power"], target)
    assert info_a.keys() - {"target_power"} == info_b.keys()
    for name in info_b:
        assert _same(info_a[name], info_b[name]), name


def test_env_with_a_profile_steps_as_a_twin_fed_its_rows():
    from nuclear_sim_amd.env import PowerProfile
    n, steps = 515, 48
    seeds = 100 + np.arange(n)
    kw = dict(noise_enabled=True, noise_seeds=seeds, noise_generator="device")
    dev = _env(n, power_profile=dict(seeds=seeds, steps=steps, base_power_percent=98.0, noise_std_percent=0.2, block=37), **kw)
    twin = _env(n, **kw)
    rows = PowerProfile(twin, seeds, steps, 98.0, 0.2)
    explicit = torch.full((n,), 95.0, dtype=torch.float64, device=dev.device)
    for t in range(130):
        if t == 70:           # a reset of the whole batch re-seeds the profile, as it re-seeds the noise
            _same_step((dev.reset(), dev._reward, dev._done, {}), (twin.reset(), twin._reward, twin._done, {}))
            rows = PowerProfile(twin, seeds, steps, 98.0, 0.2)
        if t in (20, 21, 90):  # a column the caller passes wins and consumes no row
            _same_step(dev.step(power_setpoint=explicit), twin.step(power_setpoint=explicit))
            continue
        sp, tg = rows.next()
        _same_step(dev.step(), twin.step(power_setpoint=sp), target=tg)
    fa, ia = dev.state_arrays()
    fb, ib = twin.state_arrays()
    assert _same(fa, fb) and _same(ia, ib)
    dev.close(); twin.close()


def test_the_profile_continues_across_an_autoreset():
    from nuclear_sim_amd.env import BatchedPlantEnv, PowerProfile
    seeds, steps = list(range(300)), 20
    kw = dict(autoreset=True, max_episode_steps=steps, noise_generator="device")
    dev = BatchedPlantEnv.action_test("oil_top_off", seeds, power_profile_steps=steps, **kw)
    twin = BatchedPlantEnv.action_test("oil_top_off", seeds, **kw)
    rows = PowerProfile(twin, seeds, steps)        # the composer's 90 / 2.0 profile, seeded with the scenario seeds
    for t in range(45):
        sp, tg = rows.next()
        ra, rb = dev.step(), twin.step(power_setpoint=sp)
        _same_step(ra, rb, target=tg)
        if t % steps == 0:                          # every truncated plant's next episode begins exactly with the next profile
            assert _same(sp, tg)
        if t % steps == steps - 1:
            assert bool(ra[3]["truncated"].any())
    dev.close(); twin.close()


def test_state_moves_to_a_new_handle_mid_profile():
    from nuclear_sim_amd.env import PowerProfile
    n, steps = 300, 48
    seeds = 7 + np.arange(n)
    a_env, b_env = _env(n), _env(n)
    a = PowerProfile(a_env, seeds, steps, 98.0, 0.2, block=10)
    for _ in range(30):
        a.next()                                   # three blocks of ten: position 30 of the first profile
    state = a.get_state()
    assert state[5] == 30
    b = PowerProfile(b_env, np.zeros(n, dtype=np.int64), steps, 98.0, 0.2, block=10)
    b.next()                                       # a block under way is dropped by set_state
    b.set_state(*state)
    ra, rb = a.fill(70, with_draws=True), b.fill(70, with_draws=True)
    for x, y in zip(ra, rb):
        assert _same(x, y)
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    a_env.close(); b_env.close()


def test_one_batch_gives_the_rows_of_two_handles():
    from nuclear_sim_amd.env import PowerProfile
    n, cut, steps = 600, 350, 48
    seeds = 1000 + np.arange(n)
    base = np.where(np.arange(n) % 2 == 0, 90.0, 98.0)
    whole, left, right = _env(n), _env(cut), _env(n - cut)
    w = PowerProfile(whole, seeds, steps, base, 2.0).fill(100)
    l = PowerProfile(left, seeds[:cut], steps, base[:cut], 2.0).fill(100)
    r = PowerProfile(right, seeds[cut:], steps, base[cut:], 2.0).fill(100)
    for k in range(2):
        assert _same(w[k], torch.cat([l[k], r[k]], dim=1))
    for e in (whole, left, right):
        e.close()


def test_refusals():
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import PowerProfile
    n = 64
    env = _env(n)
    L, h = env.L, env._h
    out = torch.empty((4, n), dtype=torch.float64, device=env.device)
    ptr = ctypes.c_void_p(out.data_ptr())
    with pytest.raises(_lib.NpbError):       # fill before seed
        _lib.check(L.npb_profile_fill(h, 4, ptr, None, None, env._stream()), h)
    key, pos, has, cached, carried = (np.zeros((n, 624), dtype=np.uint32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32),
                                      np.zeros(n), np.zeros((5, n)))
    with pytest.raises(_lib.NpbError):       # state before seed
        _lib.check(L.npb_profile_set_state(h, *(a.ctypes.data_as(ctypes.c_void_p) for a in (key, pos, has, cached, carried)), 0, env._stream()), h)
    with pytest.raises(_lib.NpbError):
        PowerProfile(env, [2 ** 32] + [0] * (n - 1), 10)
    with pytest.raises(_lib.NpbError):
        PowerProfile(env, [-1] + [0] * (n - 1), 10)
    with pytest.raises(ValueError):
        PowerProfile(env, range(n), 0)
    with pytest.raises(ValueError):
        PowerProfile(env, range(n - 1), 10)
    with pytest.raises(ValueError):
        PowerProfile(env, range(n), 10, base_power_percent=[90.0, 98.0])
    s = np.arange(n, dtype=np.int64)
    two = np.array([90.0, 98.0])
    with pytest.raises(_lib.NpbError):       # steps < 1, and a column of neither one nor n values, at the C ABI itself
        _lib.check(L.npb_profile_seed(h, s.ctypes.data_as(ctypes.c_void_p), 0, None, 0, None, 0, env._stream()), h)
    with pytest.raises(_lib.NpbError):
        _lib.check(L.npb_profile_seed(h, s.ctypes.data_as(ctypes.c_void_p), 10, two.ctypes.data_as(ctypes.c_void_p), 2, None, 0, env._stream()), h)
    with pytest.raises(_lib.NpbError):       # still nothing seeded
        _lib.check(L.npb_profile_fill(h, 4, ptr, None, None, env._stream()), h)
    g = PowerProfile(env, range(n), 10)
    with pytest.raises(_lib.NpbError):       # k = 0
        _lib.check(L.npb_profile_fill(h, 0, ptr, None, None, env._stream()), h)
    with pytest.raises(_lib.NpbError):       # no setpoint block
        _lib.check(L.npb_profile_fill(h, 4, None, ptr, None, env._stream()), h)
    with pytest.raises(_lib.NpbError):       # the ramp: k < 1 with blocks, and a NULL block
        _lib.check(L.npb_profile_ramp(h, 0, ptr, ptr, env._stream()), h)
    with pytest.raises(_lib.NpbError):
        _lib.check(L.npb_profile_ramp(h, 4, ptr, None, env._stream()), h)
    with pytest.raises(_lib.NpbError):
        _lib.check(L.npb_profile_ramp(h, 4, None, ptr, env._stream()), h)
    g.next()
    state = g.get_state()
    names = ("key", "pos", "has_gauss", "cached", "carried", "position")
    for bad in ({"pos": np.full(n, 625)}, {"pos": np.full(n, -1)}, {"has_gauss": np.full(n, 2)}, {"position": 10}, {"position": -1}):
        args = dict(zip(names, state))
        args.update(bad)
        with pytest.raises(_lib.NpbError):
            g.set_state(**args)
    after = g.get_state()                     # a refused state leaves the profile alone
    for x, y in zip(state, after):
        assert np.array_equal(x, y)
    env.close()
