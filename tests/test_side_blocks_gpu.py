"""The state beside the arena -- the component maintenance's side state and the carried diagnostics rows -- with BOTH blocks on at once,
through every episode path: masked restore from a bank of another pitch, masked restore from the snapshot, the autoreset from either,
and the refusals.  72 plants (pitch 128: a full and a partial wave) restore from a bank of 8 (pitch 64), under either storage type.
Everything is compared on the bit patterns."""
import ctypes
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, M, ADVANCE = 72, 8, 3
SLOTS = (5 * np.arange(N)) % M
MASK = np.arange(N) % 3 == 0          # plants of the full wave and of the partial one, and plants of each left out
WHAT = ("f64", "i32", "component maintenance state", "diagnostics state")


def _env(n, storage="f64", **kw):
    from nuclear_sim_amd.env import BatchedPlantEnv
    both = dict(maintenance=True, component_maintenance=True, diagnostics=True)
    both.update(kw)
    return BatchedPlantEnv(n, dt=5.0, storage=storage, **both)


def _state(env):
    """a plant's three things: the arena (two arrays), the component maintenance's side state, the carried diagnostics rows"""
    f, i = env.state_arrays()
    return f, i, env.component_maintenance_state(), env.diagnostics_state()


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _assert_same(got, want, where):
    for g, w, what in zip(got, want, WHAT):
        assert torch.equal(_bits(g), _bits(w)), "%s: %s differs" % (where, what)


def _cols(state, index):
    index = torch.as_tensor(np.asarray(index), device=state[0].device)
    return tuple(t[:, index] for t in state)


def _steps(env, k):
    """k steps that leave every plant of the batch in a state of its own"""
    for _ in range(k):
        out = env.step(power_setpoint=80.0 + 0.25 * np.arange(env.n))
    return out


def _marked(rows, n, device):
    """a finite value of its own in every row of every plant: a restore that takes the wrong entry, or the wrong row, shows"""
    return (1000.0 * torch.arange(rows, dtype=torch.float64, device=device)[:, None]
            + torch.arange(n, dtype=torch.float64, device=device)[None, :] + 0.5)


def _mark_side_blocks(env):
    """overwrite both side blocks of every plant with marked values (the env is not stepped afterwards)"""
    from nuclear_sim_amd import _lib
    env.load_component_maintenance_state(_marked(_lib.CMAINT_SIDE_DOUBLES, env.n, env.device))
    env.load_diagnostics_state(-_marked(len(_lib.DIAG_CARRIED_ROWS), env.n, env.device))


def _pair(storage):
    """the target, three steps into its run, and a bank whose entries differ in the arena and in every row of both blocks"""
    target, bank = _env(N, storage), _env(M, storage)
    _steps(target, 3)
    _steps(bank, 4)
    _mark_side_blocks(bank)
    entries = _state(bank)
    assert all(len({tuple(col) for col in _bits(t).T.tolist()}) == M for t in (entries[0], entries[2], entries[3]))
    return target, bank, entries


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_masked_restore_from_a_bank_of_another_pitch(storage):
    target, bank, entries = _pair(storage)
    before = _state(target)
    target.set_start_bank(bank, slots=SLOTS, advance=ADVANCE)
    target.restore_from_bank(MASK)
    got = _state(target)
    _assert_same(_cols(got, np.flatnonzero(MASK)), _cols(entries, SLOTS[MASK]), "masked plants hold their bank entries")
    _assert_same(_cols(got, np.flatnonzero(~MASK)), _cols(before, np.flatnonzero(~MASK)), "the other plants are unchanged")
    nxt, start = target.next_start_slots.cpu().numpy(), target.episode_start.cpu().numpy()
    assert np.array_equal(nxt[MASK], (SLOTS[MASK] + ADVANCE) % M) and np.array_equal(nxt[~MASK], SLOTS[~MASK])
    assert np.array_equal(start[MASK], SLOTS[MASK]) and (start[~MASK] == -1).all()
    target.close(); bank.close()


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_masked_restore_from_the_snapshot(storage):
    target = _env(N, storage)
    _steps(target, 3)
    target.snapshot()
    snap = _state(target)
    _steps(target, 3)
    stepped = _state(target)
    assert not torch.equal(_bits(stepped[0]), _bits(snap[0])) and not torch.equal(_bits(stepped[3]), _bits(snap[3]))
    target.restore(MASK)
    got = _state(target)
    _assert_same(_cols(got, np.flatnonzero(MASK)), _cols(snap, np.flatnonzero(MASK)), "masked plants hold the snapshot")
    _assert_same(_cols(got, np.flatnonzero(~MASK)), _cols(stepped, np.flatnonzero(~MASK)), "the other plants hold the stepped state")
    # ... and with every row of both blocks drifted away from the snapshot's, whatever the three steps did to them
    _mark_side_blocks(target)
    drifted = _state(target)
    target.restore(MASK)
    got = _state(target)
    _assert_same(_cols(got, np.flatnonzero(MASK)), _cols(snap, np.flatnonzero(MASK)), "masked plants hold the snapshot (marked rows)")
    _assert_same(_cols(got, np.flatnonzero(~MASK)), _cols(drifted, np.flatnonzero(~MASK)), "the other plants keep the marked rows")
    target.close()


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("source", ["snapshot", "bank"])
def test_autoreset_after_a_truncation(storage, source):
    target, bank, entries = _pair(storage)
    if source == "bank":
        target.set_start_bank(bank, slots=SLOTS, advance=ADVANCE)
        want = _cols(entries, SLOTS)
    else:
        target.snapshot()
        want = _state(target)
    target._enable_autoreset(2)
    _obs, _rew, done, info = _steps(target, 1)
    assert not info["truncated"].any() and not done.any()
    _obs, _rew, done, info = _steps(target, 1)
    assert info["truncated"].all() and not done.any()
    _assert_same(_state(target), want, "every plant holds its source entry after the truncation (%s)" % source)
    if source == "bank":
        assert np.array_equal(target.episode_start.cpu().numpy(), SLOTS)
        assert np.array_equal(target.next_start_slots.cpu().numpy(), (SLOTS + ADVANCE) % M)
    target.close(); bank.close()


def _raises(text):
    from nuclear_sim_amd import _lib
    return pytest.raises(_lib.NpbError, match=re.escape(text))


def test_refusals_keep_their_texts():
    from nuclear_sim_amd import _lib
    # a snapshot taken before a block was switched on does not hold it
    a = _env(M, component_maintenance=False, diagnostics=False)
    a.snapshot()
    table = _lib.NpbComponentMaintTable()
    a.L.npb_default_component_maintenance_table(ctypes.byref(table))
    _lib.check(a.L.npb_set_component_maintenance(a._h, ctypes.byref(table)), a._h)
    with _raises("the component maintenance is on (npb_set_component_maintenance) and the snapshot was taken without it: npb_snapshot again"):
        a.restore()
    b = _env(M, component_maintenance=False, diagnostics=False)
    b.snapshot()
    b.enable_diagnostics(True, carried=True)
    with _raises("the diagnostics rows are carried (npb_carry_diagnostics) and the snapshot was taken without them: npb_snapshot again"):
        b.restore()
    # a bank handle that lacks a block; lacking both, the diagnostics rows are named
    target = _env(N)
    no_cm, no_diag, neither = _env(M, component_maintenance=False), _env(M, diagnostics=False), _env(M, component_maintenance=False, diagnostics=False)
    with _raises("npb_set_start_bank: this handle has the component maintenance on (npb_set_component_maintenance) and the bank handle has not"):
        target.set_start_bank(no_cm)
    for bank in (no_diag, neither):
        with _raises("npb_set_start_bank: this handle carries the diagnostics rows (npb_carry_diagnostics) and the bank handle does not"):
            target.set_start_bank(bank)
    for e in (a, b, target, no_cm, no_diag, neither):
        e.close()
