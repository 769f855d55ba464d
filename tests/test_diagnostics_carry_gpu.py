"""GPU: the diagnostics rows the step carries in the caller's buffer (include/npb.h NPB_DIAG_CARRIED; BatchedPlantEnv(diagnostics=True),
npb_carry_diagnostics) travel with snapshots, start banks, the autoreset, resets and checkpoints, and the state log tells episodes
apart.  Reference values: the reference's own state logs of the l2 / l3 / m1 runs (tests/golden/log_*.npz), compared with the rule of
test_state_log_reproduces_the_references_log_column_by_column (RTOL, floor 1e-9, 1e-6 for fouling_energy_penalty_mw) on windows that
start after each fixture's last poke, so without that test's turbine-on-a-poked-step exemption."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from golden_util import Golden, GOLDEN_DIR, RTOL
from test_gpu_parity import _env, _host_state

pytestmark = pytest.mark.gpu

HISTORY = ("secondary.ph_control.ph_control_deviation_rms", "secondary.ph_control.ph_control_time_in_control",
           "secondary.feedwater_SECONDARY-COMP-001-FW.protection_npsh_trend")
_F = "secondary.feedwater_SECONDARY-COMP-001-FW."
OVERSPEED = "secondary.turbine_SECONDARY-COMP-001-TURB.overspeed_events"
ROW = {r: k for k, r in enumerate((124, 125, 126, 127, 128, 133, 141, 142, 143, 164, 165, 166, 167))}    # carried row -> its place in diagnostics_state()


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


_logs = {}


def _reference_log(name):
    """(column names, [T, 784] log) of the reference's own run of a fixture: loaded once, never written"""
    if name not in _logs:
        z = np.load(os.path.join(GOLDEN_DIR, "log_%s.npz" % name))
        log = z["log"]; log.setflags(write=False)
        _logs[name] = ([str(x) for x in z["names"]], log)
    return _logs[name]


def _load0(env, g):
    """the fixture's initial state into every lane"""
    f0, i0 = _host_state(env)
    f, i, fm, im = g.split_state(g.state[0])
    f0[fm, :] = f[fm, None]; i0[im, :] = i[im, None]
    env.load_state_arrays(f0, i0)


def _step(env, g, t):
    """the fixture's step t (0-based), its pokes first, the same inputs for every lane"""
    for label, v in g.pokes.get(t, []):
        kind, slot = g.label_slot(label)
        env._set_slot(kind, slot, np.full(env.n, v))
    sp = None if np.isnan(g.setpoint[t]) else g.setpoint[t]
    cw = None if np.isnan(g.cooling[t]) else g.cooling[t]
    return env.step(action=int(g.action[t]), magnitude=float(g.magnitude[t]), power_setpoint=sp, cooling_water_temp=cw, noise_z=float(g.noise_z[t]))


def _compare(tab, names, lanes, want_rows, ref_names, ref):
    """table rows (sample i, lane j) against ref[want_rows[i, j]] for every column of `names`; want_rows < 0 = not compared"""
    ns = want_rows.shape[0]
    compared = 0
    for name in names:
        mine = tab[name].to_numpy().reshape(ns, len(lanes))
        col = ref[:, ref_names.index(name)]
        floor = 1e-6 if name.endswith("fouling_energy_penalty_mw") else 1e-9
        sel = want_rows >= 0
        want = col[np.where(sel, want_rows, 0)]
        ok = (np.abs(mine - want) <= RTOL * np.abs(want) + floor) | ~sel
        assert ok.all(), (name, np.argwhere(~ok)[:3].tolist(), mine[~ok][:3], want[~ok][:3])
        compared += int(sel.sum())
    return compared


def _state(env):
    f, i = env.state_arrays()
    return f, i


def _wave_mask(n):
    """the lanes p % 3 == 1 of the first wave, no lane of a later one: the first wave's restore is partial, the others leave early"""
    m = np.zeros(n, dtype=np.uint8)
    m[1:64:3] = 1
    return m


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("fixture,s", [("l2_feedwater_events_log", 46), ("l3_turbine_sg_events_log", 32), ("m1_oil_top_off_staggered", 20)])
def test_mid_run_snapshot_and_masked_restore_replay_the_references_log(fixture, s):
    """Snapshot a plant s steps into the fixture's run, run on to T, restore the masked lanes and replay steps s+1..T: the restored lanes
    reproduce the reference's log rows s+1..T in every column but the three history windows (781 of 784) -- the carried diagnostics
    columns included, which a restore that puts a fresh plant's values reads as 0 / 1.0 -- and the other lanes equal, to the bit, a
    control batch that never restored."""
    from nuclear_sim_amd import statelog
    g = Golden(fixture)
    ref_names, ref = _reference_log(fixture)
    T, n = g.T, 128
    assert max(g.pokes, default=-1) < s and ref.shape == (T, 784)
    # non-vacuity, from the reference's own log: the carried quantities have moved by the snapshot step
    at = lambda key, step: ref[step - 1, ref_names.index([c for c in ref_names if c.endswith(key)][0])]
    assert np.array_equal(ref[:, ref_names.index(OVERSPEED)], np.arange(1, T + 1))
    if fixture.startswith("l2"):
        assert at("protection_valid_trip_count", 46) == 1.0 and at("protection_emergency_feedwater", 46) == 1.0
    if fixture.startswith("l3"):
        assert abs(at("SJE-002_compression_ratio", 32) - 14.43) < 0.005
        assert abs(at("SJE-001_operating_hours", 32) - 1.5) < 1e-9 and abs(at("SJE-002_operating_hours", 32) - 1.167) < 5e-4
    E, C = _env(g, n=n, diagnostics=True), _env(g, n=n, diagnostics=True)
    for env in (E, C):
        _load0(env, g)
    for t in range(s):
        _step(E, g, t); _step(C, g, t)
    assert E.last_step_kernel() == "npb_step_diag_kernel"
    E.snapshot()
    at_snapshot = E.diagnostics_state()
    for t in range(s, T):
        _step(E, g, t); _step(C, g, t)
    mask = _wave_mask(n)
    E.restore(mask)
    m = torch.as_tensor(mask.astype(bool), device=E.device)
    assert _same(E.diagnostics_state()[:, m], at_snapshot[:, m]) and float(E.diagnostics_state()[ROW[128], 1].item()) == s
    log = statelog.StateLog(E, every=1, capacity=T - s, diagnostics=True)
    outs = None
    for t in range(s, T):
        outs = (_step(E, g, t), _step(C, g, t))
        log.record(t + 1, (t + 1) * E.dt)
    # the lanes that were not restored: a control that never restored, to the bit
    (fe, ie), (fc, ic) = _state(E), _state(C)
    assert _same(fe[:, ~m], fc[:, ~m]) and _same(ie[:, ~m], ic[:, ~m])
    for k in (0, 1, 2):
        assert _same(outs[0][k][~m], outs[1][k][~m]), k
    assert _same(E.diagnostics[:, ~m], C.diagnostics[:, ~m])
    assert not _same(E.diagnostics[:, m], C.diagnostics[:, m])
    # the restored lanes: the reference's rows s+1..T, all columns but the history windows
    lanes = [1, 31, 61]
    tab = log.table(plants=lanes)
    produced = [c for c in tab.column_names if c not in ("step", "time", "plant")]
    assert sorted(produced) == sorted(set(ref_names) - set(HISTORY)) and len(produced) == 781
    want = np.repeat(np.arange(s, T)[:, None], len(lanes), axis=1)
    assert _compare(tab, produced, lanes, want, ref_names, ref) == 781 * (T - s) * len(lanes)
    assert _same(fe[:, 1], fe[:, 61]) and _same(E.diagnostics[:, 1], E.diagnostics[:, 61])     # every restored lane is the same plant
    E.close(); C.close()


# ---------------------------------------------------------------------------------------------------------------- B
def test_autoreset_with_staggered_lanes_logs_every_episode_as_the_reference_run():
    """m1 from its initial state, autoreset with max_episode_steps = 24, inputs per plant by its own episode step; restore(mask) at
    global step 7 staggers the p % 3 == 1 lanes of wave 0, so every later truncation there is a partial-wave reset.  80 steps, a
    StateLog of every step: `episode` / `episode_step` are the integer sequences the schedule implies, and every row with
    episode_step = k >= 1 is the reference's log row k - 1 in all 784 columns, the per-episode history windows included."""
    from nuclear_sim_amd import statelog
    g = Golden("m1_oil_top_off_staggered")
    ref_names, ref = _reference_log("m1_oil_top_off_staggered")
    assert not g.pokes
    n, K, steps = 128, 24, 80
    env = _env(g, n=n, diagnostics=True, autoreset=True, max_episode_steps=K)
    _load0(env, g)
    env.snapshot()
    obs0 = env.get_observation().clone()
    log = statelog.StateLog(env, every=1, capacity=steps, diagnostics=True)
    mask = _wave_mask(n)
    own = np.zeros(n, dtype=np.int64)          # each lane's own episode step (steps taken since its last restart)
    episode = np.zeros(n, dtype=np.int64)
    want_episode, want_step = [], []
    for t in range(steps):
        if t == 7:
            env.restore(mask)
            own[mask != 0] = 0; episode[mask != 0] += 1
        obs, reward, done, info = env.step(action=g.action[own].astype(np.int32), magnitude=g.magnitude[own], power_setpoint=g.setpoint[own],
                                           noise_z=g.noise_z[own])
        log.record(t + 1, (t + 1) * env.dt)
        ends = own + 1 == K
        assert not bool(done.any())
        assert np.array_equal(info["truncated"].cpu().numpy().astype(bool), ends), t
        assert np.array_equal(info["episode_length"].cpu().numpy(), own + 1), t
        assert np.array_equal(info["episode_index"].cpu().numpy(), episode), t         # the episode this transition belonged to
        o = obs.cpu().numpy()
        e = torch.as_tensor(ends, device=env.device)
        if ends.any():          # the terminal observation moves to final_observation, obs shows the restored start state
            assert _same(obs[e], obs0[e]), t
            np.testing.assert_allclose(info["final_observation"].cpu().numpy()[ends], np.broadcast_to(g.obs[K - 1], (int(ends.sum()), 22)), rtol=RTOL, atol=1e-9)
        np.testing.assert_allclose(o[~ends], g.obs[own[~ends]], rtol=RTOL, atol=1e-9, err_msg=str(t))
        episode = episode + ends
        own = np.where(ends, 0, own + 1)
        want_episode.append(episode.copy()); want_step.append(own.copy())
    want_episode, want_step = np.stack(want_episode), np.stack(want_step)
    # the schedule: the rest of wave 0 and wave 1 truncate at steps 24 / 48 / 72, the restarted lanes at 31 / 55 / 79
    assert np.flatnonzero(want_step[:, 0] == 0).tolist() == [23, 47, 71] and np.flatnonzero(want_step[:, 1] == 0).tolist() == [30, 54, 78]
    assert want_episode[-1, 0] == 3 and want_episode[-1, 1] == 4 and want_episode[-1, 127] == 3
    lanes = [0, 1, 2, 61, 63, 64, 127]
    tab = log.table(plants=lanes)
    assert str(tab["episode"].type) == "int64" and str(tab["episode_step"].type) == "int64"
    assert np.array_equal(tab["episode"].to_numpy().reshape(steps, len(lanes)), want_episode[:, lanes])
    assert np.array_equal(tab["episode_step"].to_numpy().reshape(steps, len(lanes)), want_step[:, lanes])
    produced = [c for c in tab.column_names if c not in ("step", "time", "plant", "episode", "episode_step")]
    assert sorted(produced) == sorted(ref_names) and len(produced) == 784
    want = want_step[:, lanes] - 1          # episode_step k >= 1 -> the reference's row k - 1; step-0 rows (-1) are not compared
    compared = _compare(tab, produced, lanes, want, ref_names, ref)
    assert compared == 784 * int((want >= 0).sum()) and (want >= 0).sum() >= (steps - 4) * len(lanes)
    for name in HISTORY:        # the windows are NaN on the mixed rows only
        v = tab[name].to_numpy().reshape(steps, len(lanes))
        assert np.array_equal(np.isnan(v), want < 0), name
    env.close()


def test_state_log_of_an_autoreset_env_needs_the_rows_carried():
    from nuclear_sim_amd import statelog, _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv(64, autoreset=True, max_episode_steps=5)
    with pytest.raises(_lib.NpbError, match="diagnostics=True"):
        statelog.StateLog(env, diagnostics=True)
    log = statelog.StateLog(env, capacity=4)          # without diagnostics the log works, with the episode columns
    for t in range(4):
        env.step()
        log.record(t + 1, t + 1.0)
    tab = log.table(plants=[0, 63])
    assert tab["episode_step"].to_numpy().tolist() == [1, 1, 2, 2, 3, 3, 4, 4] and not tab["episode"].to_numpy().any()
    plain = BatchedPlantEnv(64)
    plain.step()
    log = statelog.StateLog(plain, capacity=1)
    log.record(1, 1.0)
    assert "episode" not in log.table().column_names and "episode_step" not in log.table().column_names
    env.close(); plain.close()


# ---------------------------------------------------------------------------------------------------------------- C
def test_start_bank_entries_bring_their_carried_rows():
    """A carrying bank batch 46 steps into the l2 run; a carrying target restores lane p from entry (7 p) % 64: the rows arrive from
    the entry, not the lane, and the restored lanes replay steps 47..60 as the reference logged them."""
    from nuclear_sim_amd import statelog, _lib
    g = Golden("l2_feedwater_events_log")
    ref_names, ref = _reference_log("l2_feedwater_events_log")
    s, T, M, n = 46, g.T, 64, 128
    bank = _env(g, n=M, diagnostics=True)
    _load0(bank, g)
    for t in range(s):
        _step(bank, g, t)
    target = _env(g, n=n, diagnostics=True)
    for t in range(3):
        _step(target, g, t)
    before = target.diagnostics_state()
    slots = (7 * np.arange(n)) % M
    mask = _wave_mask(n)
    m = torch.as_tensor(mask.astype(bool), device=target.device)
    # entries told apart by a row the run leaves at rest (the steam-dump latch): the restore must index the bank by entry
    honest = bank.diagnostics_state()
    marked = honest.clone()
    marked[ROW[143]] = torch.arange(M, dtype=torch.float64, device=bank.device) + 0.5
    bank.load_diagnostics_state(marked)
    target.set_start_bank(bank, slots=slots)
    target.restore_from_bank(mask)
    got = target.diagnostics_state()
    assert _same(got[:, m], marked[:, torch.as_tensor(slots, device=bank.device)][:, m]) and _same(got[:, ~m], before[:, ~m])
    assert got[ROW[143], 1].item() == 7.5 and got[ROW[141], 1].item() == 1.0 and got[ROW[128], 1].item() == s
    # ... and the run goes on from the entry as the reference's did
    bank.load_diagnostics_state(honest)
    target.set_start_bank(bank, slots=slots)
    target.restore_from_bank(mask)
    log = statelog.StateLog(target, every=1, capacity=T - s, diagnostics=True)
    for t in range(s, T):
        _step(target, g, t)
        log.record(t + 1, (t + 1) * target.dt)
    lanes = [1, 31, 61]
    tab = log.table(plants=lanes)
    produced = [c for c in tab.column_names if c not in ("step", "time", "plant")]
    assert sorted(produced) == sorted(set(ref_names) - set(HISTORY)) and len(produced) == 781
    want = np.repeat(np.arange(s, T)[:, None], len(lanes), axis=1)
    assert _compare(tab, produced, lanes, want, ref_names, ref) == 781 * (T - s) * len(lanes)
    # a bank that does not carry the rows has nothing to give a target that does
    plain = _env(g, n=M)
    with pytest.raises(_lib.NpbError, match="carries the diagnostics rows .* the bank handle does not"):
        target.set_start_bank(plain)
    bank.close(); target.close(); plain.close()


# ---------------------------------------------------------------------------------------------------------------- D
def test_checkpoint_of_a_diagnostics_env_is_the_arrays_and_the_diagnostics_state():
    g = Golden("m1_oil_top_off_staggered")
    n = 70
    A = _env(g, n=n, diagnostics=True)
    _load0(A, g)
    for t in range(20):
        _step(A, g, t)
    f, i = A.state_arrays()
    ds = A.diagnostics_state()
    assert tuple(ds.shape) == (13, n) and ds.dtype == torch.float64
    assert bool((ds[ROW[128]] == 20.0).all()) and bool((ds[ROW[166]] > 1.6).all())
    B, B2 = _env(g, n=n, diagnostics=True), _env(g, n=n, diagnostics=True)
    B.load_state_arrays(f, i); B.load_diagnostics_state(ds)
    B2.load_state_arrays(f, i)                  # the arrays alone: the carried columns restart
    outs = None
    for t in range(20, 30):
        outs = [_step(env, g, t) for env in (A, B, B2)]
    (fa, ia), (fb, ib) = _state(A), _state(B)
    assert _same(fa, fb) and _same(ia, ib)
    for k in (0, 1, 2):
        assert _same(outs[0][k], outs[1][k]), k
    assert _same(A.diagnostics, B.diagnostics)
    assert bool((A.diagnostics[128] == 30.0).all()) and bool((B2.diagnostics[128] == 10.0).all())
    assert not _same(A.diagnostics, B2.diagnostics)
    # a row no fixture moves (the steam-dump latch, 143) survives get / set and snapshot / restore
    ds = A.diagnostics_state()
    ds[ROW[143]] = torch.arange(n, dtype=torch.float64, device=A.device) * 0.25 + 1.0
    A.load_diagnostics_state(ds)
    assert _same(A.diagnostics_state(), ds) and _same(A.diagnostics[143], ds[ROW[143]])
    A.snapshot()
    zeroed = ds.clone(); zeroed[ROW[143]] = 0.0
    A.load_diagnostics_state(zeroed)
    _step(A, g, 30)
    assert not bool(A.diagnostics[143].any())
    A.restore()
    assert _same(A.diagnostics_state(), ds)
    with pytest.raises(ValueError):
        A.load_diagnostics_state(ds[:, :-1])
    for env in (A, B, B2):
        env.close()


# ---------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("segment", [None, 64])
@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_restore_puts_back_the_snapshots_rows_under_either_storage_and_on_a_segmented_arena(storage, segment, monkeypatch):
    """n = 192: with NPB_ARENA_SEGMENT=64 three segments of 64 plants, whose waves index the unsegmented diagnostics buffer by the global
    plant number.  Every lane carries its own values, so a row restored from or into the wrong lane shows."""
    from nuclear_sim_amd.env import BatchedPlantEnv
    if segment:
        monkeypatch.setenv("NPB_ARENA_SEGMENT", str(segment))
    else:
        monkeypatch.delenv("NPB_ARENA_SEGMENT", raising=False)
    n = 192
    E, C = (BatchedPlantEnv(n, storage=storage, diagnostics=True) for _ in range(2))
    assert int(E.L.npb_state_arena_segment(E._h)) == (segment or 0)
    lane = torch.arange(n, dtype=torch.float64, device=E.device)
    for env in (E, C):
        ds = env.diagnostics_state()
        for r in (124, 125, 126, 127, 128, 141, 143, 166, 167):
            ds[ROW[r]] = lane * (r - 120) + r
        env.load_diagnostics_state(ds)
    for t in range(5):
        E.step(power_setpoint=95.0); C.step(power_setpoint=95.0)
    E.snapshot()
    at_snapshot = E.diagnostics_state()
    fs, is_ = E.state_arrays()
    for t in range(5):
        E.step(power_setpoint=90.0); C.step(power_setpoint=90.0)
    mask = np.zeros(n, dtype=np.uint8)
    mask[1:64:3] = 1; mask[128:192] = 1; mask[130] = 0          # a partial wave, an untouched one, a nearly whole one
    m = torch.as_tensor(mask.astype(bool), device=E.device)
    assert not _same(E.diagnostics_state()[:, m], at_snapshot[:, m])
    E.restore(mask)
    got = E.diagnostics_state()
    assert _same(got[:, m], at_snapshot[:, m])
    assert _same(got[:, ~m], C.diagnostics_state()[:, ~m]) and _same(E.diagnostics[:, ~m], C.diagnostics[:, ~m])
    assert got[ROW[128], 190].item() == 190 * 8 + 128 + 5 and got[ROW[128], 130].item() == 130 * 8 + 128 + 10
    (fe, ie), (fc, ic) = _state(E), _state(C)
    assert _same(fe[:, m], fs[:, m]) and _same(ie[:, m], is_[:, m]) and _same(fe[:, ~m], fc[:, ~m]) and _same(ie[:, ~m], ic[:, ~m])
    E.close(); C.close()


# ---------------------------------------------------------------------------------------------------------------- F
def test_resets_put_the_fresh_and_the_references_values_on_the_masked_lanes_only():
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 100
    golden = json.load(open(os.path.join(GOLDEN_DIR, "diag_carry", "reference_reset.json")))["rows"]
    assert [r["row"] for r in golden] == list(_lib.DIAG_CARRIED_ROWS)
    env = BatchedPlantEnv(n, diagnostics=True)
    assert [float(v) for v in env.diagnostics_state()[:, n - 1].tolist()] == list(_lib.DIAG_CARRIED_ROWS.values())
    moved = torch.rand((13, n), dtype=torch.float64, device=env.device) + 2.0        # no row's fresh or reset value
    mask = (np.arange(n) % 4 == 2).astype(np.uint8)
    m = torch.as_tensor(mask.astype(bool), device=env.device)
    env.load_diagnostics_state(moved)
    env.reset(mask)
    got = env.diagnostics_state()
    assert _same(got[:, ~m], moved[:, ~m])
    for k, (row, fresh) in enumerate(_lib.DIAG_CARRIED_ROWS.items()):
        assert bool((got[k, m] == fresh).all()), row
    env.load_diagnostics_state(moved)
    env.reset(mask, reference=True)
    got = env.diagnostics_state()
    assert _same(got[:, ~m], moved[:, ~m])
    kept = 0
    for k, r in enumerate(golden):
        if r["rule"] == "kept":
            assert _same(got[k, m], moved[k, m]), r["row"]
            kept += 1
        else:
            assert bool((got[k, m] == r["reset_to"]).all()), (r["row"], r["reset_to"])
    assert kept == 2       # what the live reference showed: the two compression ratios
    env.reset()            # the whole batch
    assert bool((env.diagnostics_state() == torch.tensor(list(_lib.DIAG_CARRIED_ROWS.values()), device=env.device)[:, None]).all())
    env.close()


def test_refusals():
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    a = BatchedPlantEnv(64)
    L, h = a.L, a._h
    buf = torch.zeros((13, 64), dtype=torch.float64, device=a.device)
    with pytest.raises(_lib.NpbError, match="no diagnostics buffer"):
        _lib.check(L.npb_carry_diagnostics(h, 1), h)
    with pytest.raises(_lib.NpbError, match="not carried"):
        a.diagnostics_state()
    with pytest.raises(_lib.NpbError, match="not carried"):
        a.load_diagnostics_state(buf)
    # a snapshot, and a bank, taken before the rows were carried do not hold them
    a.snapshot()
    a.set_start_bank(a)
    a.enable_diagnostics(True, carried=True)
    with pytest.raises(_lib.NpbError, match="diagnostics .* start bank was set without"):
        _lib.check(L.npb_set_autoreset(h, 1, 0), h)
    with pytest.raises(_lib.NpbError, match="start bank was set without"):
        a.restore_from_bank()
    a.set_start_bank(None)
    with pytest.raises(_lib.NpbError, match="diagnostics .* snapshot was taken without"):
        _lib.check(L.npb_set_autoreset(h, 1, 0), h)
    with pytest.raises(_lib.NpbError, match="snapshot was taken without"):
        a.restore()
    # replacing the buffer while its rows are carried
    other = torch.zeros((_lib.DIAG_DIM, 64), dtype=torch.float64, device=a.device)
    with pytest.raises(_lib.NpbError, match="carried"):
        _lib.check(L.npb_set_diagnostics(h, ctypes.c_void_p(other.data_ptr()), 64), h)
    with pytest.raises(_lib.NpbError, match="carried"):
        a.enable_diagnostics()
    a.snapshot()
    _lib.check(L.npb_set_autoreset(h, 1, 0), h)          # accepted: carrying, and the snapshot holds the rows
    with pytest.raises(_lib.NpbError, match="autoreset is on"):
        _lib.check(L.npb_set_diagnostics(h, ctypes.c_void_p(other.data_ptr()), 64), h)
    with pytest.raises(_lib.NpbError, match="autoreset is on"):
        _lib.check(L.npb_set_diagnostics(h, None, 0), h)
    with pytest.raises(_lib.NpbError, match="autoreset is on"):
        _lib.check(L.npb_carry_diagnostics(h, 0), h)
    _lib.check(L.npb_set_autoreset(h, 0, 0), h)
    _lib.check(L.npb_carry_diagnostics(h, 0), h)
    with pytest.raises(_lib.NpbError, match="not carried"):
        a.diagnostics_state()
    # without carrying the handle is where it was: diagnostics and autoreset exclude each other, with the old message
    with pytest.raises(_lib.NpbError, match="carries plant state the snapshot does not hold"):
        _lib.check(L.npb_set_autoreset(h, 1, 0), h)
    a.enable_diagnostics(False)
    # a target that carries and a bank that does not
    b = BatchedPlantEnv(64, diagnostics=True)
    with pytest.raises(_lib.NpbError, match="the bank handle does not"):
        b.set_start_bank(a)
    a.close(); b.close()
