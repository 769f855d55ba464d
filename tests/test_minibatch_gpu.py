"""GPU: the pinned moments, the keyed permutation and the minibatch gather over a recorded rollout (npb_rollout_moments,
npb_rollout_permutation, npb_rollout_minibatch; BatchedPlantEnv.rollout_moments / rollout_permutation / rollout_minibatches).

The reference is nuclear_sim_amd.rollout, the numpy statement (held to its own words on the CPU in test_minibatch_cpu.py), fed with the
device's recorded tensors.  Sums in a pinned order, a division, a root, integer mixing and copies: every comparison is by bits (view(int32)
/ view(int64)), with no tolerance anywhere.  One exception in kind, not in width: of a NaN result only "it is a NaN" is compared, a NaN's
payload being no part of the statement.

The run is the rollout suite's: action_test("oil_top_off", range(n), dt=5.0, autoreset=True, max_episode_steps=3) with n = 300 -- ragged
against a wave of 64 and a workgroup of 256, and two partials, so the finish kernel's tree runs -- recorded as a prefix of t = 5 of T = 8
slots (N = 1500, neither a power of two nor of four: the walk is exercised) and then fully (N = 2400)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DT, T, N_PLANTS, L_MAX = 5.0, 8, 300, 3
POKES = {1: [5, 66, 100], 2: [9, 64, 129], 4: [11, 200], 5: [20, 69, 299]}
COLUMNS = [(("pump.oil_level", 0), {"ref": 50.0, "scale": 0.02}), ("reward", {"scale": 0.5, "fresh": 0.0}), ("obs", 3), ("prim.fuel_temperature", {"scale": 1e-3})]
AXES = [("rod", "rate"), ("valve", "rate", {"scale": 0.5}), (None, "value")]


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(a):
    a = np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a)
    return a.view(np.int32) if a.dtype == np.float32 else a.view(np.int64) if a.dtype == np.float64 else a


def _same(got, want, where):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (where, g.shape, w.shape, g.dtype, w.dtype)
    assert np.array_equal(g, w), (where, np.argwhere(g != w)[:4].tolist())


def _setpoint(t, n):
    return 90.0 + 8.0 * np.sin(2.0 * np.pi * t / (20.0 + np.arange(n) % 7))


def _env(C=4, K=2, dtype=torch.float32, controls=True, n=N_PLANTS):
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, autoreset=True, max_episode_steps=L_MAX)
    env.set_features(COLUMNS[:C], stack=K, dtype=dtype, final=True)
    if controls:
        env.set_controls(AXES)
    return env


def _step(env, t, extras):
    """step t of the rollout suite's run: its poke, the policy's random and reproducible controls and extras, the step"""
    plants = [p for p in POKES.get(t, ()) if p < env.n]
    if plants:
        v = _np(env.get_field("prim.fuel_temperature"))
        v[plants] = 1500.0
        env.set_field("prim.fuel_temperature", v)
    before = _np(env.features())
    g = torch.Generator().manual_seed(1000 + t)
    act = extra = None
    if env._ctl is not None:
        act = (2.0 * torch.rand(env.controls_input().shape, generator=g) - 1.0).to(env.controls_input().dtype)
        env.controls_input().copy_(act)
    if extras:
        extra = (0.25 * torch.rand((env.n, extras), generator=g)).to(torch.float32)
        env.rollout_extras_input().copy_(extra)
    return before, act, extra, env.step(power_setpoint=_setpoint(t, env.n))


def _advantages(env, dtype):
    g = torch.Generator().manual_seed(7)
    n, R = env.n, env.rollout_spec()["final_rows"]
    values = (torch.rand((T, n), generator=g) - 0.5).to(torch.float32)
    return env.rollout_advantages(0.99, 0.95, values=values, last_value=(torch.rand(n, generator=g) - 0.5).to(torch.float32),
                                  final_values=(torch.rand(n * R, generator=g) - 0.5).to(torch.float32), dtype=dtype)


def _same_moments(got, want, where):
    got, want = _np(got), np.array(want, dtype=np.float64)
    assert got.shape == (4,) and got.dtype == np.float64
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (where, got, want)
    assert np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64)), (where, got, want)


def _check_epoch(env, arrays, t, adv, ret, unit, batch, normalise, seed, epoch, **kw):
    """every minibatch of one epoch against the numpy statement, and the epoch's indices tiling range(N) exactly once"""
    from nuclear_sim_amd import rollout
    N = t * env.n if unit == "transition" else env.n
    a, r = _np(adv), _np(ret)
    m = rollout.moments(a[:t]) if normalise else None
    keys = rollout.permutation_keys(seed, epoch)
    first, seen = 0, []
    for mb in env.rollout_minibatches(batch, seed=seed, first_epoch=epoch, normalize=normalise, unit=unit, advantages=(adv, ret), **kw):
        count = min(batch, N - first)
        assert mb["epoch"] == epoch and mb["index"].shape == (count,) and mb["index"].dtype == torch.int32
        want = rollout.minibatch(arrays, t, a, r, keys, first, count, unit, moments=m, eps=1e-8)
        for name in ("index", "obs", "act", "extra", "adv", "ret"):
            if want[name] is None:
                assert mb[name] is None, name
            else:
                _same(mb[name], want[name], (name, unit, batch, first, str(adv.dtype), normalise))
        seen.append(want["index"])
        first += count
    assert first == N and np.array_equal(np.sort(np.concatenate(seen)), np.arange(N, dtype=np.int32))
    return len(seen)


# ---------------------------------------------------------------------------------------------------------------- 1
# (K, C) = (2, 4) float32: 32-byte rows, the 16-byte path; (1, 3) float32: the element path; (2, 4) float64: 64-byte rows.  With controls
# (A = 3: 12- and 24-byte rows) and extras (E = 2: 8-byte rows), and with neither.
CASES = [(2, 4, torch.float32, True, 2), (1, 3, torch.float32, False, 0), (2, 4, torch.float64, True, 2)]


@pytest.mark.parametrize("K, C, dtype, controls, E", CASES)
def test_minibatches_bit_for_bit_with_the_numpy_statement(K, C, dtype, controls, E):
    """Both units, float32 and float64 advantages, with and without the moments, batch sizes 64, 97 (a short last batch of 45 at N =
    1500) and N, over the prefix t = 5 and the full T = 8.  Fails without the feature: rollout_minibatches does not exist"""
    from nuclear_sim_amd import rollout
    env = _env(C, K, dtype, controls)
    env.set_rollout(T, extras=E)
    with pytest.raises(Exception, match="rollout_advantages"):      # no advantages formed yet: refused, naming the call, before any launch
        env.rollout_minibatches(64)
    done_t = 0
    for t in (5, T):
        for s in range(done_t, t):
            _step(env, s, E)
        done_t = t
        r = env.rollout()
        assert r["t"] == t
        arrays = {k: (None if r[k] is None else _np(r[k])) for k in ("obs", "act", "extra")}
        for adv_dtype in (torch.float32, torch.float64):
            adv, ret = _advantages(env, adv_dtype)
            assert adv.shape == (t, env.n)
            _same_moments(env.rollout_moments(), rollout.moments(_np(adv)), ("adv", t))
            for unit in ("transition", "plant"):
                N = t * env.n if unit == "transition" else env.n
                for batch in (64, 97, N):
                    for normalise in ((True, False) if batch == 97 else (adv_dtype == torch.float32,)):
                        made = _check_epoch(env, arrays, t, adv, ret, unit, batch, normalise, seed=3, epoch=t)
                        assert made == -(-N // batch)
                        if (unit, batch, t) == ("transition", 97, 5):
                            assert N == 1500 and N % batch == 45
    # drop_last, epochs, and the views: the same storage on every yield
    adv, ret = _advantages(env, torch.float32)
    got = list(env.rollout_minibatches(97, epochs=2, seed=1, first_epoch=4, drop_last=True))
    assert len(got) == 2 * (T * env.n // 97) and [m["epoch"] for m in got[::len(got) // 2]] == [4, 5]
    assert all(m["obs"].data_ptr() == got[0]["obs"].data_ptr() and m["index"].shape == (97,) for m in got)
    env.set_rollout(None)      # drops the buffers with the rollout
    with pytest.raises(Exception, match="set_rollout"):
        env.rollout_minibatches(64)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.fixture(scope="module")
def small():
    """70 plants, 4 of 8 slots recorded, float32 advantages: what the tests below share"""
    env = _env(n=70)
    env.set_rollout(T, extras=1)
    for s in range(4):
        _step(env, s, 1)
    adv, ret = _advantages(env, torch.float32)
    yield env, adv, ret
    env.close()


def test_moments_of_tensors_not_bound_to_n(small):
    """[2, 65 836]: 258 partials and then 2: a third tree level; [5, 1]: no tree; [1, 257]: a second group that is nearly all padding; a
    NaN propagates; float64 as float32.  No rollout is needed: a twin handle without one gives the same bits"""
    from nuclear_sim_amd import rollout
    env = small[0]
    g = torch.Generator().manual_seed(11)
    shapes = [((2, 65536 + 300), torch.float32, 1), ((5, 1), torch.float32, 1), ((1, 257), torch.float32, 0), ((1, 1), torch.float64, 0),
              ((3, 300), torch.float64, 2), ((9, 513), torch.float32, 1)]
    for shape, dtype, ddof in shapes:
        x = (torch.randn(shape, generator=g, dtype=torch.float64) * 3.0 + 0.5).to(dtype).to(env.device)
        got = env.rollout_moments(x, ddof=ddof)
        assert got.device == env.device and got.dtype == torch.float64
        _same_moments(got, rollout.moments(_np(x), ddof), (shape, str(dtype)))
        _same_moments(env.rollout_moments(x, ddof=ddof), rollout.moments(_np(x), ddof), (shape, "again"))      # the same bits again
    x = torch.ones((3, 300), dtype=torch.float32)
    x[1, 299] = float("nan")
    want = rollout.moments(_np(x))
    assert want[0] == 900.0 and np.isnan(want[1])
    _same_moments(env.rollout_moments(x.to(env.device)), want, "a NaN")
    x[1, 299] = float("inf")
    _same_moments(env.rollout_moments(x.to(env.device)), rollout.moments(_np(x)), "an infinity")
    for bad, ddof in ((torch.zeros((2, 3)), 6), (torch.zeros((2, 3)), -1), (torch.zeros(5), 1), (torch.zeros((2, 2), dtype=torch.int32), 1)):
        with pytest.raises(ValueError):
            env.rollout_moments(bad.to(env.device), ddof=ddof)
    from nuclear_sim_amd import _lib      # the library's own refusal, before any launch
    d = _lib.NpbMomentsDesc()
    keep = torch.zeros(8, dtype=torch.float64, device=env.device)
    d.src, d.type, d.ddof, d.rows, d.cols, d.out = keep.data_ptr(), 1, 4, 2, 2, keep.data_ptr() + 32
    assert env.L.npb_rollout_moments(env._h, ctypes.byref(d), None) == -1 and b"ddof" in env.L.npb_last_error(env._h)
    d.ddof, d.type = 1, 7
    assert env.L.npb_rollout_moments(env._h, ctypes.byref(d), None) == -1 and b"unknown type" in env.L.npb_last_error(env._h)


def test_permutation_windows_at_large_N(small):
    """windows of 4096 entries at N = 2^23 + 1 (the domain jumps to 2^24: three of four positions walk) and N = 2^28: no big buffers"""
    from nuclear_sim_amd import rollout
    env = small[0]
    for N in (2 ** 23 + 1, 2 ** 28, 1, 5):
        keys = rollout.permutation_keys(17, N % 5)
        for first in sorted({0, N // 2, max(N - 4096, 0)}):
            count = min(4096, N - first)
            got = env.rollout_permutation(N, keys, first, count)
            assert got.dtype == torch.int32
            _same(got, rollout.permutation(N, keys, first, count), (N, first))
    for N, first, count, why in ((0, 0, 1, b"N must be"), (2 ** 31, 0, 1, b"N must be"), (10, 5, 6, b"inside"), (10, -1, 2, b"inside"), (10, 0, 0, b"count")):
        k = (ctypes.c_uint32 * 6)(1, 2, 3, 4, 5, 6)
        out = torch.zeros(8, dtype=torch.int32, device=env.device)
        assert env.L.npb_rollout_permutation(env._h, N, k, first, count, out.data_ptr(), None) == -1 and why in env.L.npb_last_error(env._h)


def test_the_same_keys_give_the_same_bits_whatever_the_workgroup_count(small):
    env, adv, ret = small
    t = env.rollout()["t"]

    def epoch(unit, seed=5, **kw):
        return [{k: _np(v) for k, v in mb.items() if isinstance(v, torch.Tensor)} for mb in
                env.rollout_minibatches(97, seed=seed, first_epoch=2, unit=unit, **kw)]
    for unit in ("transition", "plant"):
        first = epoch(unit)
        assert len(first) == -(-(t * env.n if unit == "transition" else env.n) // 97)
        for other in (epoch(unit), epoch(unit, max_blocks=1), epoch(unit, max_blocks=2)):      # 1: one workgroup strides over every tile
            assert len(other) == len(first)
            for a, b in zip(first, other):
                assert set(a) == set(b)
                for k in a:
                    _same(a[k], b[k], (unit, k))
        assert any((a["index"] != b["index"]).any() for a, b in zip(first, epoch(unit, seed=6)))


def test_refusals_on_a_live_handle_before_any_launch(small):
    from nuclear_sim_amd import _lib
    env, adv, ret = small
    for kw, why in ((dict(batch_size=0), "batch_size"), (dict(batch_size=8, unit="episode"), "unit"), (dict(batch_size=8, eps=-1.0), "eps"),
                    (dict(batch_size=8, advantages=(adv, ret.double())), "adv's type"), (dict(batch_size=8, advantages=(adv[:2], ret[:2])), "contiguous")):
        with pytest.raises(ValueError, match=why):
            env.rollout_minibatches(**kw)
    index = torch.zeros(64, dtype=torch.int32, device=env.device)
    d = _lib.NpbMinibatchDesc()
    d.unit, d.type, d.first, d.count, d.index = 0, 0, 4 * env.n - 10, 11, index.data_ptr()
    assert env.L.npb_rollout_minibatch(env._h, ctypes.byref(d), None) == -1 and b"inside [0, N)" in env.L.npb_last_error(env._h)
    d.first, d.count, d.index = 0, 8, None
    assert env.L.npb_rollout_minibatch(env._h, ctypes.byref(d), None) == -1 and b"index is NULL" in env.L.npb_last_error(env._h)
    assert not _np(index).any()
    bare = _env(n=70, controls=False)      # no rollout set; and one with nothing recorded
    d.index = index.data_ptr()
    assert bare.L.npb_rollout_minibatch(bare._h, ctypes.byref(d), None) == -1 and b"no rollout set" in bare.L.npb_last_error(bare._h)
    with pytest.raises(Exception, match="set_rollout"):
        bare.rollout_minibatches(8)
    bare.set_rollout(T)
    assert bare.L.npb_rollout_minibatch(bare._h, ctypes.byref(d), None) == -1 and b"t == 0" in bare.L.npb_last_error(bare._h)
    bare.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_a_handle_that_never_calls_them_records_what_it_did_before():
    """The rollout suite's eight steps on a handle with a rollout set that never calls the new entry points: every recorded tensor by
    bits against rollout.Recorder fed by hand, as the rollout suite checks it; and a twin that forms moments and drains minibatches after
    every step records the same bits and ends in the same state"""
    from nuclear_sim_amd import rollout
    n, E = 130, 2
    env, twin = _env(n=n), _env(n=n)
    for e in (env, twin):
        e.set_rollout(T, extras=E)
    s = env.rollout_spec()
    rec = rollout.Recorder(s["horizon"], n, s["stack"], axes=s["axes"], extras=s["extras"], final_rows=s["final_rows"], autoreset=True,
                           max_episode_steps=s["max_episode_steps"])
    g = torch.Generator().manual_seed(1)
    adv, ret = (torch.randn((T, n), generator=g).to(twin.device) for _ in range(2))
    for t in range(T):
        before, act, extra, (obs, rew, done, info) = _step(env, t, E)
        over = (_np(done) != 0) | (_np(info["truncated"]) != 0)
        stack = np.where(over[:, None, None], _np(info["final_features"]), _np(info["features"]))
        rec.pre(before, _np(act), _np(extra))
        rec.post(_np(rew), _np(done), stack, episode=_np(info["episode_index"]))
        _, _, _, (t_obs, t_rew, t_done, t_info) = _step(twin, t, E)
        twin.rollout_moments(adv)
        for unit in ("transition", "plant"):
            assert len(list(twin.rollout_minibatches(64, unit=unit, advantages=(adv, ret)))) > 0
        _same(obs, t_obs, ("obs", t)); _same(rew, t_rew, ("reward", t))
        assert torch.equal(done, t_done), t
    got, other, want = env.rollout(), twin.rollout(), rec.arrays()
    assert got["t"] == other["t"] == T
    for name in ("obs", "act", "extra", "reward", "ended", "episode", "final_row", "final_obs"):
        _same(got[name], want[name], name)
        _same(other[name], want[name], (name, "the twin"))
    assert (_np(got["ended"]) == 2).any() and (_np(got["ended"]) == 1).any()
    for a, b in zip(env.state_arrays(), twin.state_arrays()):
        _same(a, b, "state")
    env.close(); twin.close()
