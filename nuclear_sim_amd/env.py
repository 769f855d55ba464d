"""Host-side mirror of the reference's simulator interface on top of the HIP stepper.

``BatchedPlantEnv`` steps N independent plants per call (one wavefront lane per plant);
``NuclearPlantSimulator`` / ``NuclearPlantEnv`` are single-plant facades with the reference's
scalar signatures (simulator/core/sim.py:27-258, 911-940) so that existing loops
(maintenance_scenario_runner.py:383-411, data/gen_training_data.py:249-290) run unchanged.

PyTorch is only the device-array container: every tensor handed to the library is passed as
a raw device pointer (``tensor.data_ptr()``).
"""
from __future__ import annotations

import ctypes
import os
import enum
import re
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib, controls, normalizer, policy, recordlog, recurrent, rollout
from .schema import SCHEMA


class ControlAction(enum.Enum):
    """systems/primary/__init__.py:28-45"""
    CONTROL_ROD_INSERT = 0
    CONTROL_ROD_WITHDRAW = 1
    INCREASE_COOLANT_FLOW = 2
    DECREASE_COOLANT_FLOW = 3
    OPEN_STEAM_VALVE = 4
    CLOSE_STEAM_VALVE = 5
    INCREASE_FEEDWATER = 6
    DECREASE_FEEDWATER = 7
    NO_ACTION = 8
    DILUTE_BORON = 9
    BORATE_COOLANT = 10
    START_FEEDWATER_PUMP = 11
    STOP_FEEDWATER_PUMP = 12
    INCREASE_FEEDWATER_PUMP_SPEED = 13
    DECREASE_FEEDWATER_PUMP_SPEED = 14


INFO_COLUMNS = ("thermal_power", "reactivity", "electrical_power", "thermal_efficiency", "steam_flow",
                "steam_pressure", "condenser_pressure", "condenser_heat_rejection", "time", "feedwater_flow",
                "sg_heat_transfer", "turbine_power", "feedwater_power", "primary_thermal_power",
                "turbine_efficiency", "turbine_hp_power", "turbine_lp_power")


assert len(INFO_COLUMNS) == _lib.INFO_DIM     # the info block's width, checked against the library itself in _lib.load()


class HeatSourceNoise:
    """Per-plant pre-drawn heat-source noise, bit-identical to the reference's
    ``np.random.RandomState(seed).normal(0, sigma)`` stream (constant_heat_source.py:58-62,178):
    numpy's legacy normal is loc + scale * gauss, so the standard-normal stream of the same
    RandomState reproduces it exactly.  Drawn on the host a block of steps at a time and uploaded as ONE
    [block, n] tensor, so a step costs no host-to-device copy (BASELINE config 3 seeds every plant differently,
    42 + i: 65 536 generators; the draw is ~8 s per 256 steps on one core and happens once per block)."""

    def __init__(self, seeds: Sequence[int], block: int = 256, device=None):
        # one generator per DISTINCT seed (the data-gen runner seeds every plant's heat source with 42, so a
        # 262 144-plant batch needs one stream, not 262 144 generator objects)
        uniq, self._index = np.unique(np.asarray(seeds, dtype=np.int64), return_inverse=True)
        self._rngs = [np.random.RandomState(int(s)) for s in uniq]
        self._block = block
        self._device = device
        self._buf = None
        self._pos = block

    def next(self):
        if self._pos >= self._block:
            draws = np.stack([r.standard_normal(self._block) for r in self._rngs])          # [distinct seeds, block]
            host = np.ascontiguousarray(draws[self._index].T)                                 # [block, n]
            self._buf = host if self._device is None else torch.from_numpy(host).to(self._device)
            self._pos = 0
        out = self._buf[self._pos]
        self._pos += 1
        return out


class DeviceHeatSourceNoise:
    """``HeatSourceNoise`` generated on the device: one Mersenne Twister per plant, owned by ``env``'s handle (npb_noise_seed),
    that follows ``np.random.RandomState(seed).standard_normal()`` -- the integer state exactly, every draw within a few ulp (only
    the fp64 log is the device library's).  ``next()`` hands out one [n] float64 device row per call and refills a
    [block, n] block with npb_noise_fill when it runs out.  Each refill is a fresh tensor from torch's stream-ordered allocator, so
    rows handed out earlier stay valid, as they do with the host class.

    ``get_state()`` / ``set_state()`` use numpy's ``get_state()`` layout (key [n, 624] uint32, pos, has_gauss, cached).  The state is
    the generators' -- after the current block, not after the last row handed out; ``set_state`` drops the rest of the block.
    The generators belong to the handle: a second instance on the same env re-seeds them."""

    def __init__(self, env: "BatchedPlantEnv", seeds: Sequence[int], block: int = 256):
        if int(block) < 1:
            raise ValueError("block must be >= 1")
        s = np.ascontiguousarray(np.asarray(seeds, dtype=np.int64).reshape(-1))
        if s.size != env.n:
            raise ValueError("one seed per plant: %d seeds for %d plants" % (s.size, env.n))
        self._env = env
        self._block = int(block)
        _lib.check(env.L.npb_noise_seed(env._h, s.ctypes.data_as(ctypes.c_void_p), env._stream()), env._h)
        self._buf = None
        self._pos = self._block

    def next(self) -> torch.Tensor:
        env = self._env
        env._refuse_in_episode_streams("DeviceHeatSourceNoise.next()")
        if self._pos >= self._block:
            with torch.cuda.device(env.device):
                self._buf = torch.empty((self._block, env.n), dtype=torch.float64, device=env.device)
            _lib.check(env.L.npb_noise_fill(env._h, self._block, ctypes.c_void_p(self._buf.data_ptr()), env._stream()), env._h)
            self._pos = 0
        out = self._buf[self._pos]
        self._pos += 1
        return out

    def get_state(self):
        """(key [n, 624] uint32, pos [n] int32, has_gauss [n] int32, cached [n] float64) of every plant's generator"""
        env, n = self._env, self._env.n
        key = np.empty((n, 624), dtype=np.uint32)
        pos, has_gauss = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        cached = np.empty(n, dtype=np.float64)
        _lib.check(env.L.npb_noise_get_state(env._h, *(a.ctypes.data_as(ctypes.c_void_p) for a in (key, pos, has_gauss, cached)),
                                             env._stream()), env._h)
        return key, pos, has_gauss, cached

    def set_state(self, key, pos, has_gauss, cached) -> None:
        """load every plant's generator state (numpy's layout, as ``get_state`` returns it); the rest of the block is dropped"""
        env, n = self._env, self._env.n
        env._refuse_in_episode_streams("DeviceHeatSourceNoise.set_state()")
        arrays = (np.ascontiguousarray(np.broadcast_to(np.asarray(key, dtype=np.uint32), (n, 624))),
                  np.ascontiguousarray(np.broadcast_to(np.asarray(pos, dtype=np.int32), (n,))),
                  np.ascontiguousarray(np.broadcast_to(np.asarray(has_gauss, dtype=np.int32), (n,))),
                  np.ascontiguousarray(np.broadcast_to(np.asarray(cached, dtype=np.float64), (n,))))
        _lib.check(env.L.npb_noise_set_state(env._h, *(a.ctypes.data_as(ctypes.c_void_p) for a in arrays), env._stream()), env._h)
        self._buf = None
        self._pos = self._block


class PowerProfile:
    """The data-gen runner's power profile, drawn on the device per plant (npb_profile_seed / npb_profile_fill): what
    ``MaintenanceScenarioRunner._generate_power_profile(steps)`` and ``_set_target_power`` (maintenance_scenario_runner.py:586-671)
    make of ``np.random.normal(0, 1, steps)`` -- noise of min(0.2, std) % around the base power clipped to [20, 105] %, a 3-point
    moving average, at most 0.05 % a step, then the heat source's ramp of at most 0.02 % a step -- for a stream seeded per plant
    (``RandomState(seed)``) just before the runner draws.  ``scenarios.power_profile_rows`` is the same in numpy.  The generators are
    a second set in ``env``'s handle, independent of the heat-source noise's.  ``base_power_percent`` / ``noise_std_percent`` are
    scalars or one value per plant (the composer's template has 90 / 2.0 and 98 / 0.2 profiles; a fleet may mix them).

    ``next()`` hands out ``(setpoint_row, target_row)``, [n] float64 device rows: the setpoint is what ``step(power_setpoint=...)``
    takes, the target what the runner logs as target_power.  A [block, n] block is refilled when it runs out; each refill is a fresh
    tensor, so rows handed out earlier stay valid.  After ``steps`` rows the next profile of the same horizon begins from the next
    draw, its ramp afresh (the first setpoint is the first target), as a second runner in the same process would.

    ``get_state()`` / ``set_state()``: the generators in numpy's ``get_state()`` layout, the filter's carried values [5, n] and the
    position in the current profile.  As with ``DeviceHeatSourceNoise`` the state is the handle's -- after the current block, not
    after the last row handed out -- and ``set_state`` drops the rest of the block; it belongs on a ``PowerProfile`` built with the
    same ``steps`` and load profiles.  A second instance on the same env re-seeds the handle's profile."""

    def __init__(self, env: "BatchedPlantEnv", seeds: Sequence[int], steps: int, base_power_percent=90.0, noise_std_percent=2.0,
                 block: int = 256):
        if int(block) < 1:
            raise ValueError("block must be >= 1")
        if int(steps) < 1:
            raise ValueError("steps must be >= 1")
        if not hasattr(env.L, "npb_profile_seed"):
            raise _lib.NpbError("libnpb.so has no npb_profile_seed (older than ABI 152): rebuild")
        s = np.ascontiguousarray(np.asarray(seeds, dtype=np.int64).reshape(-1))
        if s.size != env.n:
            raise ValueError("one seed per plant: %d seeds for %d plants" % (s.size, env.n))
        cols = []
        for name, v in (("base_power_percent", base_power_percent), ("noise_std_percent", noise_std_percent)):
            a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
            if a.size not in (1, env.n):
                raise ValueError("%s: one value, or one per plant (%d for %d plants)" % (name, a.size, env.n))
            cols.append(a)
        self._env = env
        self._block = int(block)
        self.steps = int(steps)
        _lib.check(env.L.npb_profile_seed(env._h, s.ctypes.data_as(ctypes.c_void_p), self.steps,
                                          cols[0].ctypes.data_as(ctypes.c_void_p), cols[0].size,
                                          cols[1].ctypes.data_as(ctypes.c_void_p), cols[1].size, env._stream()), env._h)
        self._buf = None
        self._pos = self._block

    def fill(self, k: int, with_draws: bool = False):
        """the next ``k`` rows as fresh [k, n] tensors ``(setpoint, target)`` -- with ``with_draws`` also the draw behind each row's raw
        value, ``(setpoint, target, z)``: ``scenarios.power_profile_rows(z)`` of a whole profile equals the other two bit for bit"""
        env = self._env
        env._refuse_in_episode_streams("PowerProfile.fill()")
        with torch.cuda.device(env.device):
            out = torch.empty((3 if with_draws else 2, int(k), env.n), dtype=torch.float64, device=env.device)
        _lib.check(env.L.npb_profile_fill(env._h, int(k), ctypes.c_void_p(out[0].data_ptr()), ctypes.c_void_p(out[1].data_ptr()),
                                          ctypes.c_void_p(out[2].data_ptr()) if with_draws else None, env._stream()), env._h)
        return tuple(out)

    def next(self):
        self._env._refuse_in_episode_streams("PowerProfile.next()")
        if self._pos >= self._block:
            self._buf = self.fill(self._block)
            self._pos = 0
        out = self._buf[0][self._pos], self._buf[1][self._pos]
        self._pos += 1
        return out

    def get_state(self):
        """(key [n, 624] uint32, pos [n] int32, has_gauss [n] int32, cached [n] float64, carried [5, n] float64, position); with
        episode streams on the position is -1: every plant has its own (``BatchedPlantEnv.profile_positions()``)"""
        env, n = self._env, self._env.n
        key = np.empty((n, 624), dtype=np.uint32)
        pos, has_gauss = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        cached, carried = np.empty(n, dtype=np.float64), np.empty((5, n), dtype=np.float64)
        position = ctypes.c_int32(0)
        _lib.check(env.L.npb_profile_get_state(env._h, *(a.ctypes.data_as(ctypes.c_void_p) for a in (key, pos, has_gauss, cached, carried)),
                                               ctypes.byref(position), env._stream()), env._h)
        return key, pos, has_gauss, cached, carried, int(position.value)

    def set_state(self, key, pos, has_gauss, cached, carried, position) -> None:
        """load a state as ``get_state`` returns it; the rest of the block is dropped"""
        env, n = self._env, self._env.n
        env._refuse_in_episode_streams("PowerProfile.set_state()")
        arrays = (np.ascontiguousarray(np.broadcast_to(np.asarray(key, dtype=np.uint32), (n, 624))),
                  np.ascontiguousarray(np.broadcast_to(np.asarray(pos, dtype=np.int32), (n,))),
                  np.ascontiguousarray(np.broadcast_to(np.asarray(has_gauss, dtype=np.int32), (n,))),
                  np.ascontiguousarray(np.broadcast_to(np.asarray(cached, dtype=np.float64), (n,))),
                  np.ascontiguousarray(np.broadcast_to(np.asarray(carried, dtype=np.float64), (5, n))))
        _lib.check(env.L.npb_profile_set_state(env._h, *(a.ctypes.data_as(ctypes.c_void_p) for a in arrays), int(position), env._stream()), env._h)
        self._buf = None
        self._pos = self._block


NOISE_GENERATORS = ("host", "device")


def equilibrium_state(power_level=100.0, control_rod_position=95.0) -> Dict[str, object]:
    """create_equilibrium_state(power_level, control_rod_position, auto_balance=True)  reactivity_model.py:443-529, as a field
    dict for ``BatchedPlantEnv.set_fields``.  Scalars, or arrays [n] for one state per plant (BASELINE config 2: power ~ U[60, 100] %,
    rods ~ U[80, 100] % per plant): temperatures and precursors follow the asked power level, the boron concentration is the
    critical one for the asked rod position at those temperatures (calculate_critical_boron_concentration :390-416 on
    calculate_total_reactivity :77-125 with boron = 0) -- and the last two lines of the reference put flux and power level back to
    exactly 100 % whatever was asked (:518-520), which is reproduced."""
    p = np.asarray(power_level, dtype=np.float64); rods = np.asarray(control_rod_position, dtype=np.float64)
    p, rods = np.broadcast_arrays(p, rods)
    beta = [0.000215, 0.001424, 0.001274, 0.002568, 0.000748, 0.000273]
    lam = [0.077, 0.311, 1.40, 3.87, 1.40, 0.195]
    flux = 1e13 * (p / 100.0)
    prec = [(beta[i] / lam[i]) * (flux / 1e-5) for i in range(6)]
    fuel_t = 575.0 + (p - 100.0) * 2.0
    cool_t = 293.0 + (17.0 * (p / 100.0))
    # total reactivity without boron (ReactivityModel.calculate_total_reactivity, boron = 0), the dict's ten terms in their order
    pos = np.minimum(np.maximum(rods / 100.0, 0.0), 1.0)
    comps = [3000.0 * (pos - 0.5), -10.0 * 0.0, -2.5e-5 * (fuel_t - 575.0) * 1e5, -3.0e-5 * (cool_t - 280.0) * 1e5,
             -1000.0 * 0.0, 0.5 * (15.5 - 15.5), (1.0e15 / 1.0e15) * -1800.0, (5.0e14 / 5.0e14) * -600.0,
             3340.0 + -0.15 * 15000.0, 0.0 * float(np.exp(-0.0002 * 15000.0))]
    total = 0
    for c in comps:
        total = total + c
    boron = np.maximum(0, (total - 0.0) / -10.0)
    one = np.ones_like(p)
    d = {"prim.neutron_flux": 1e13 * one, "prim.power_level": 100.0 * one, "prim.control_rod_position": rods * one,
         "prim.xenon_concentration": 1.0e15 * one, "prim.iodine_concentration": 1.5e16 * one,
         "prim.samarium_concentration": 5.0e14 * one, "prim.fuel_temperature": fuel_t,
         "prim.coolant_temperature": cool_t, "prim.boron_concentration": boron}
    for i in range(6):
        d[("prim.precursors", 0, i)] = prec[i]
    if p.ndim == 0:
        d = {k: float(v) for k, v in d.items()}
    return d


def config2_draws(n: int):
    """BASELINE config 2's per-plant (power level, rod position) draws: U[60, 100] % and U[80, 100] % from
    numpy.random.default_rng(1234) -- one generator per quantity (1234, 1235), each indexed by plant, so that plant i's state does not
    depend on how many plants the batch has"""
    return np.random.default_rng(1234).uniform(60.0, 100.0, n), np.random.default_rng(1235).uniform(80.0, 100.0, n)


class BatchedPlantEnv:
    """N plants behind the reference's step()/reset()/observation contract, as columns.

    step() returns ``(obs[N,22], reward[N], done[N], info)`` where ``info`` holds column tensors
    (``electrical_power``, ``trip_flags``, ...) instead of one dict per plant.

    Every tensor step() hands out -- obs, reward, done and each column of info, ``info["maintenance_event_count"]`` included (the
    column the step kernels keep current, npb_set_maintenance_count_buffer) -- is one of the env's own device buffers, written again
    by the next step: ``clone()`` what is to be kept (a list that appends them step after step holds N aliases of the latest values).

    Episodes (no reference counterpart; gymnasium's vector-env "same-step" autoreset): ``snapshot()`` records every plant's
    episode-start state on the device -- call it AFTER ``set_fields`` has put the initial conditions in -- and ``restore(mask)``
    puts the masked plants back to it.  ``autoreset=True`` snapshots the construction state and has every step() put plants whose
    episode ended (``done``, or ``max_episode_steps`` steps: truncation, which termination wins over) back to the snapshot in the
    same step, on the device: ``obs`` then holds the restored observation for them, while reward, done and the rest of ``info``
    describe the terminal transition; ``info`` gains ``truncated``, ``final_observation`` (this step's obs of the reset plants;
    other rows are stale), ``episode_length`` and ``episode_return`` (as of this step: a reset plant's finished episode).  Only the
    plant state in the arena is restored: the pre-drawn heat-source noise stream (``HeatSourceNoise``) continues across an
    autoreset (its filter state, in the arena, is restored) -- unless ``episode_streams=True`` (below).  With autoreset ``info["episode_index"]`` numbers each plant's episodes
    (the episode this step's transition belonged to; every restart, ``restore`` and ``reset`` included, starts the next).

    Diagnostics with episodes: the diagnostics build of the step (``enable_diagnostics``; the state log's step-internal columns) keeps
    thirteen values per plant from one step to the next in the diagnostics buffer, not in the arena (``_lib.DIAG_CARRIED_ROWS``:
    bearing clearance, overspeed events, the stage system's efficiency, the feedwater protection's trip count and latches, the
    ejectors' compression ratio and hours).  ``diagnostics=True`` switches the diagnostics on with these rows CARRIED
    (npb_carry_diagnostics) before the first snapshot: ``snapshot`` / ``restore``, the start bank, the autoreset and the resets then
    take them along on the device, and ``diagnostics_state()`` / ``load_diagnostics_state()`` checkpoint them.  A plain
    ``enable_diagnostics()`` does not carry them: it and autoreset exclude each other (the diagnostics buffer carries plant state the
    snapshot does not hold), and ``restore`` puts the rows back to a freshly constructed plant's, whatever the snapshot was taken from.

    Start bank: ``set_start_bank(bank_env)`` copies another batch's states (M plants, any M) into a bank the handle owns; from then
    on the autoreset, and ``restore_from_bank(mask)``, restore a plant from bank entry ``next_start_slots[p] mod M`` instead of its
    own snapshot lane, and advance its slot, all on the device.  ``info["episode_start"]`` is the bank entry of the episode each
    step's transition belonged to (-1: not from the bank), ``episode_start`` the entry of each plant's last bank restore.  A
    restored plant takes the entry's clock and maintenance stamps; the heat-source noise stream stays with the plant position.

    Operator-ordered maintenance: ``perform_maintenance(action, pump, mask=...)`` is the reference's
    ``pump.perform_maintenance(type, **kwargs)`` for the whole batch, between two steps, on the device (npb_perform_maintenance): the
    caller decides when a feedwater pump is serviced, with the automatic maintenance off or beside it.
    ``perform_component_maintenance(component, action, unit=..., mask=...)`` is the same for the steam generators, the
    steam-generator system, the condenser and its steam-jet ejectors (npb_perform_component_maintenance): TSP and scale cleaning,
    moisture-separator work, condenser cleaning and water treatment, leak repair, ejector cleaning and nozzle replacement.

    Automatic maintenance of steam generators and condenser: ``component_maintenance=True`` (with ``maintenance=True``, full mode) has
    the three generators and the condenser scanned and maintained in ONE work-order queue with the feedwater pumps, as the reference's
    AutoMaintenanceSystem does (npb_set_component_maintenance): rows tsp_fouling_fraction / tube_wall_temperature / steam_quality per
    generator and fouling_resistance on the condenser, one shared order counter, one due order per check -- which also changes when a
    pump's order is carried out.  ``component_thresholds={"steam_generator": {...}, "condenser": {...}}`` replaces the composer's rows
    (the reference's thresholds dicts, ``_lib.component_maint_table_from_thresholds``).  Its per-plant state lives in a side buffer
    (``component_maintenance_state()`` / ``load_component_maintenance_state()``): resets, ``snapshot`` / ``restore``, the autoreset
    and the start bank take it along; a checkpoint must save it beside ``state_arrays()``.  Off by default: nothing changes.

    Work-order summary: ``enable_maintenance_summary(keys, since_minutes=...)`` has the device fold the maintenance events into four
    numbers per (key, plant) -- when the first matching work order was created and when the first was completed, and how many were
    (npb_set_maintenance_summary) -- which is what the data-gen runner returns of a finished scenario and what its timing optimiser
    reads of a probe run.  ``maintenance_summary()`` returns them as ``[n_keys, n]`` device tensors, the env's own buffers as ``info``
    is, current after every ``step`` and ``perform_*_maintenance`` call and never synchronised; nothing overflows and nothing needs
    draining, however long the run.  ``step()`` puts nothing new into ``info``.  Output only, like the event log: ``snapshot``,
    ``restore``, the autoreset and the start bank leave it alone, ``clear_maintenance_summary(mask)`` starts plants afresh.
    ``nuclear_sim_amd.timing`` builds the optimiser's question on it: ``trigger_times`` for a batch of probes, ``sweep`` for the search.

    Heat-source noise (``noise_enabled``): ``noise_generator="host"`` (the default) draws each plant's
    ``RandomState(seed).standard_normal()`` stream on the host (``HeatSourceNoise``); ``"device"`` generates the same streams on the
    device (``DeviceHeatSourceNoise``: integer state exactly numpy's, every draw within a few ulp), with no host work per step.
    Either way ``reset()`` of the whole batch re-seeds seeded streams; a masked reset, ``restore`` and the autoreset keep them going.

    Power profile (``power_profile=dict(seeds=..., steps=..., base_power_percent=90.0, noise_std_percent=2.0, block=256)``): the
    data-gen runner's load profile and ramp drawn on the device per plant (``PowerProfile``), so that an episode needs no per-step
    host input.  ``step()`` with ``power_setpoint=None`` then takes the next row as its setpoint and returns the pre-ramp row, what
    the runner logs, as ``info["target_power"]``; an explicit ``power_setpoint`` wins, consumes no row and gives no
    ``info["target_power"]``.  ``reset()`` of the whole batch re-seeds the profile, as it re-seeds the noise; a masked reset,
    ``restore``, the start bank and the autoreset leave it running, as they leave the noise stream: all plants share one position
    in the profile.  With ``max_episode_steps == steps`` a truncated plant's next episode therefore begins exactly with the next
    profile (a plant that ends earlier restarts mid-profile, unless ``episode_streams=True``).  ``ramp_setpoints(targets)`` is the
    ramp stage alone, for targets of the caller's own.

    Episode streams (``episode_streams=True``; needs ``autoreset=True`` and, with noise, ``noise_generator="device"``): each plant's
    noise stream and power profile restart with its episode (npb_set_episode_streams), so that every (plant, episode) is the run a
    fresh env of that scenario would make, as the data-gen runner builds a new heat source and draws a new profile for every run.  The
    handle then owns the streams: ``step()`` passes no column unless the caller gives one (which wins and consumes no row, as before),
    every plant has its own position in its profile, and wherever a plant's episode index is bumped -- the autoreset, ``restore``,
    ``restore_from_bank``, ``reset`` -- its generators are seeded anew and the rows drawn ahead for it are made again from the new
    streams, on the device.  A restart from a bank entry ``s`` takes ``bank_noise_seeds[s]`` / ``bank_profile_seeds[s]`` where
    ``enable_episode_streams`` was given that table, every other restart the plant's own seeds, so a restart from the snapshot repeats
    the plant's first episode.  ``stream_rows`` holds the rows the last step took (``noise``, ``setpoint``, ``target``; the env's own
    buffers), ``info["target_power"]`` is its target row.  ``scenarios.episode_stream_rows`` states the contract in numpy.  The stream
    classes' ``next()`` / ``fill()`` / ``set_state()`` raise while the mode is on.  Off by default: nothing changes.

    Episode records (``enable_episode_records()``; needs ``autoreset=True``): the episode columns of ``info`` are overwritten by every
    step, so whoever wants the finished episodes would have to read ``done | truncated`` back after each.  With records on the device
    appends, behind every step, one record per plant whose episode ended on it (npb_set_episode_records) -- plant, episode index, bank
    entry, length, return, terminated / truncated, trip flags, step number, plant clock, optionally the terminal observation and the
    plant's rows of the work-order summary, which are then cleared so that the next episode's summary is its own -- and
    ``episode_records()`` drains them, sorted by (step, plant), whenever the caller chooses; ``write_episode_records(path)`` writes the
    table.  ``nuclear_sim_amd.timing.banked_trigger_times`` streams M scenarios through fewer lanes on it.  Output only; an episode
    the caller abandons (``restore``, ``restore_from_bank``, ``reset``) leaves no record.  Off by default: nothing changes.

    Column statistics (``enable_column_stats(columns, limits)``): what a plant's state did over a run or an episode, as a handful of
    numbers per (column, plant) instead of a time series -- min, max, sum and sum of squares (``colstats.moments``: mean and variance),
    the last value, and for a column with a limit the plant clock when it first went beyond it and how many samples were beyond.  A
    column is a state member, an info column, an obs column or the reward; one more launch behind every step folds the end-of-step
    sample of every plant into the env's tables (npb_set_column_stats), which ``column_stats()`` returns without synchronising;
    ``clear_column_stats(mask)`` starts the masked plants afresh and ``fold_column_stats()`` folds the current state once more on request.
    ``nuclear_sim_amd.colstats.fold`` states the fold in numpy and the device gives its bits.  With episode records on, each record
    carries the statistics of its own episode (``stat_min`` ...), and the tables restart with the episode.  Output only, like the
    work-order summary.  Off by default: nothing changes.

    Event windows (``enable_event_windows(columns, triggers, pre, post)``): what a plant looked like around a trip, a work order or a
    limit being crossed, with no state log of every plant and no watch list chosen beforehand.  Every plant keeps its last ``pre + 1 +
    post`` samples of up to 16 columns in a ring on the device; a trigger (rising trip bits, ``done``, a new work order or completion, the
    event count, a column crossing a limit) arms a capture, and ``post`` steps later -- or when the episode ends first -- the window goes
    into a record (npb_set_event_windows: one more launch behind every step, nothing read back).  ``event_windows()`` drains the records
    whenever the caller chooses, ``write_event_windows(path)`` writes them, ``clear_event_windows(mask)`` forgets the masked plants'
    history.  ``nuclear_sim_amd.eventwin.record`` states the capture in numpy and the device gives its bits.  Output only.  Off by
    default: nothing changes.
    """

    action_space_size = 15       # NuclearPlantEnv sim.py:916
    observation_space_size = 22  # sim.py:917-918

    def __init__(self, n_envs: int, dt: float = 1.0, heat_source: str = "constant", noise_enabled: bool = False,
                 noise_std_percent: float = 0.1, noise_seeds: Optional[Sequence[int]] = None,
                 mode: str = "full", device: int = 0, params: Optional[dict] = None, maintenance: bool = False,
                 storage: str = "f64", maintenance_thresholds: Optional[dict] = None, reactivity_components: bool = False,
                 integrator: str = "reference", autoreset: bool = False, max_episode_steps: Optional[int] = None,
                 noise_generator: str = "host", component_maintenance: bool = False, component_thresholds: Optional[dict] = None,
                 diagnostics: bool = False, power_profile: Optional[dict] = None, episode_streams: bool = False):
        if max_episode_steps is not None and not autoreset:
            raise ValueError("max_episode_steps needs autoreset=True")
        if episode_streams:      # refused before any device work
            self._check_episode_streams(autoreset, noise_enabled, noise_generator, noise_seeds is not None, power_profile is not None)
        if power_profile is not None:
            if heat_source == "external":
                raise ValueError("power_profile drives the heat source's setpoint: not with heat_source='external'")
            unknown = set(power_profile) - {"seeds", "steps", "base_power_percent", "noise_std_percent", "block"}
            if unknown or "seeds" not in power_profile or "steps" not in power_profile:
                raise ValueError("power_profile needs seeds and steps, and may have base_power_percent, noise_std_percent and block%s"
                                 % (": unknown %r" % sorted(unknown) if unknown else ""))
        if component_thresholds is not None and not component_maintenance:
            raise ValueError("component_thresholds needs component_maintenance=True")
        if diagnostics and mode != "full":
            raise ValueError("diagnostics needs mode='full': the diagnostics build is the full plant's step kernel")
        if component_maintenance and not (maintenance and mode == "full"):
            raise ValueError("component_maintenance needs maintenance=True and mode='full': the generators and the condenser share the pumps' work-order queue")
        component_table = None
        if component_thresholds is not None:      # an unknown parameter or action is refused before any device work
            component_table = _lib.component_maint_table_from_thresholds(component_thresholds)
        if noise_generator not in NOISE_GENERATORS:
            raise ValueError("noise_generator must be one of %r" % (NOISE_GENERATORS,))
        if not torch.cuda.is_available():
            raise _lib.NpbError("BatchedPlantEnv needs a HIP device (torch.cuda.is_available() is False); "
                                "there is no CPU fallback")
        self.L = _lib.load()
        self.n = int(n_envs)
        self.device = torch.device("cuda", device)
        p = _lib.default_params()
        p.dt = float(dt)
        # "external": a heat source the caller computes (the reference's HeatSource plugin interface, heat_source_interface.py:23-112):
        # step(thermal_power_mw=..., power_percent=...) takes the plugin's result as two input columns (include/npb_params.h)
        p.heat_source = {"constant": _lib.HEAT_CONSTANT, "reactor": _lib.HEAT_REACTOR, "external": _lib.HEAT_EXTERNAL}[heat_source]
        self.heat_source = heat_source
        p.hs_noise_enabled = int(bool(noise_enabled))
        p.hs_noise_std_percent = float(noise_std_percent)
        # "primary": NuclearPlantSimulator(enable_secondary=False) -- the primary side alone, obs[:, :12] (sim.py:155,333)
        p.mode = {"full": _lib.MODE_FULL, "primary_sg": _lib.MODE_PRIMARY_SG, "primary": _lib.MODE_PRIMARY}[mode]
        self.mode = mode
        # info["reactivity_components"] (sim.py:205) exists under the reactor heat source only; asked for, the step writes the
        # ten terms behind the info columns (include/npb.h NPB_RHO_*)
        # integrator="rk4" (BASELINE config 2; reactor heat source): the point-kinetics equations by fourth-order Runge-Kutta sub-steps
        # of 2 ms inside the step kernel instead of the reference's clipped explicit Euler -- no reference counterpart.  Classical
        # explicit RK4 while it is stable on the plant's prompt mode (h |rho - beta| / Lambda < 2, i.e. above about -350 pcm); a
        # plant below that -- deep rod insertion, every scram -- takes the L-stable implicit method of the same order for that
        # step (npd_primary.h), so the mode is stable over the whole clipped reactivity range [-0.9, 0.1].
        p.kinetics_rk4_substeps = {"reference": 0, "rk4": max(1, int(np.ceil(float(dt) / 0.002)))}[integrator]
        self._with_rho = bool(reactivity_components) and heat_source == "reactor"
        p.info_reactivity_components = int(self._with_rho)
        # automatic oil_top_off maintenance after every step, as the data-gen runner's simulator has it
        # (maintenance_scenario_runner.py:210-244); thresholds/cadence via params["maint_*"]
        p.maint_enabled = int(bool(maintenance))
        for k, v in (params or {}).items():
            setattr(p, k, v)
        self.params = p
        self.dt = float(dt)
        self._h = ctypes.c_void_p()
        # storage="f32": carried state kept as float in HBM, arithmetic still fp64 (BASELINE config 5; include/npb.h)
        self.storage = storage
        kind = {"f64": _lib.STORAGE_F64, "f32": _lib.STORAGE_F32}[storage]
        _lib.check(self.L.npb_create_storage(ctypes.byref(p), self.n, device, kind, ctypes.byref(self._h)))
        if maintenance_thresholds is not None:   # the reference's thresholds dict for a feedwater pump, in its order
            table = _lib.maint_table_from_thresholds(maintenance_thresholds)
            _lib.check(self.L.npb_set_maintenance_table(self._h, ctypes.byref(table)), self._h)
        self.component_maintenance = bool(component_maintenance)
        if component_maintenance:      # before the first snapshot (autoreset=True takes it below), so that it records the side state
            if not hasattr(self.L, "npb_set_component_maintenance"):
                raise _lib.NpbError("libnpb.so has no npb_set_component_maintenance (older than ABI 150): rebuild")
            if component_table is None:
                component_table = _lib.NpbComponentMaintTable()
                self.L.npb_default_component_maintenance_table(ctypes.byref(component_table))
            _lib.check(self.L.npb_set_component_maintenance(self._h, ctypes.byref(component_table)), self._h)
        with torch.cuda.device(self.device):
            self._obs = torch.zeros((self.n, 22), dtype=torch.float64, device=self.device)
            self._reward = torch.zeros(self.n, dtype=torch.float64, device=self.device)
            self._done = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
            self._flags = torch.zeros(self.n, dtype=torch.int32, device=self.device)
            self._info_buf = torch.zeros(self.n * (len(INFO_COLUMNS) + (_lib.INFO_NRHO if self._with_rho else 0)), dtype=torch.float64, device=self.device)
            self._info = self._info_buf[: self.n * len(INFO_COLUMNS)].view(self.n, len(INFO_COLUMNS))
            self._rho = self._info_buf[self.n * len(INFO_COLUMNS):].view(self.n, -1) if self._with_rho else None
        self._event_counts = None
        # for nuclear_sim_amd/statelog.py: how the reference names this plant's providers in its state log, and the log values its
        # constructor fixed from the initial conditions (action_test() replaces both with the data-gen composer's)
        self.log_naming = "default"
        self.log_side_columns = {"secondary.feedwater_SECONDARY-COMP-001-FW.diagnostics_total_wear": np.full(1, 60.0)}   # scenarios.log_side_columns(None)
        if p.maint_enabled and hasattr(self.L, "npb_set_maintenance_count_buffer"):
            with torch.cuda.device(self.device):
                self._event_counts = torch.zeros(self.n, dtype=torch.int32, device=self.device)
            _lib.check(self.L.npb_set_maintenance_count_buffer(self._h, ctypes.c_void_p(self._event_counts.data_ptr())), self._h)
        self._noise = None
        self._streams = None
        self.noise_generator = noise_generator
        self._noise_seeds = None if noise_seeds is None else np.asarray(noise_seeds, dtype=np.int64).copy()
        if noise_enabled and noise_seeds is not None:
            self._noise = self._make_noise(noise_seeds)
        self._profile = None
        self._profile_args = None if power_profile is None else dict(power_profile)
        if power_profile is not None:
            self._profile = PowerProfile(self, **self._profile_args)
        self._keep = []
        self._episode = None
        self._bank = None
        self._mlog = self._msum = self._erec = self._cstats = self._ewin = self._task = self._feat = self._ctl = self._ord = self._roll = self._norm = self._pol = None      # (see ``_OFF``)
        self._diag_buf = None; self.diagnostics = None; self._diag_carried = False
        if diagnostics:      # before the first snapshot (autoreset=True takes it below), so that it records the carried rows
            self.enable_diagnostics(True, carried=True)
        if autoreset:
            self.snapshot()
            self._enable_autoreset(max_episode_steps)
        if episode_streams:
            self.enable_episode_streams()

    @staticmethod
    def _check_episode_streams(autoreset, noise_enabled, noise_generator, noise_seeded, profile) -> None:
        """what ``episode_streams=True`` needs of the other keywords"""
        if not autoreset:
            raise ValueError("episode_streams needs autoreset=True: the streams restart where the plants' episodes do")
        if noise_enabled and noise_generator != "device":
            raise ValueError("episode_streams needs noise_generator='device': the host generator's pre-drawn stream cannot restart per plant on the device")
        if noise_enabled and not noise_seeded:
            raise ValueError("episode_streams needs noise_seeds: an unseeded stream has no beginning to restart from")
        if not noise_enabled and not profile:
            raise ValueError("episode_streams needs a stream to restart: noise_enabled with noise_seeds, or a power_profile")

    @classmethod
    def action_test(cls, action: str, seeds: Sequence[int], dt: float = 5.0, device: int = 0, randomize: bool = True,
                    params: Optional[dict] = None, autoreset: bool = False, max_episode_steps: Optional[int] = None,
                    bank_seeds: Optional[Sequence[int]] = None, noise_generator: str = "host",
                    maintenance_log: Optional[int] = None, component_maintenance: bool = False,
                    component_thresholds: Optional[dict] = None, diagnostics: bool = False,
                    power_profile_steps: Optional[int] = None, storage: str = "f64", episode_streams: bool = False,
                    episode_records=None) -> "BatchedPlantEnv":
        """One plant per seed, as data_gen's MaintenanceScenarioRunner builds them for
        ``compose_action_test_scenario(action, randomize=True, randomization_seed=seed)``
        (maintenance_scenario_runner.py:210-244): dt in minutes, ConstantHeatSource with 0.1 % noise seeded 42,
        automatic maintenance on, initial conditions from nuclear_sim_amd.scenarios (BASELINE config 4).  With ``autoreset`` the
        snapshot is taken after the initial conditions are in: each plant restarts from its own.  With ``bank_seeds`` later
        episodes start from a bank built as ``action_test(action, bank_seeds)`` with the same ``randomize``, ``dt`` and ``params``
        (``set_start_bank`` with its default slots): each restart draws a fresh scenario, as the data-gen runner's episodes do.
        ``noise_generator`` as for the constructor; ``maintenance_log`` = a capacity: ``enable_maintenance_log(capacity)``.
        ``component_maintenance`` / ``component_thresholds`` as for the constructor: the runner's plant has the automatic maintenance of
        the steam generators and the condenser on as well (the composer's rows by default); off by default, as before.
        ``diagnostics`` as for the constructor (the diagnostics build with its carried rows taken along: what ``StateLog(env,
        diagnostics=True)`` needs on an env with episodes); the bank of ``bank_seeds`` is built with the same flag.
        ``power_profile_steps`` = T attaches the runner's power profile of T steps (``power_profile=dict(seeds=seeds, steps=T)``: the
        composer's 90 % / 2.0 % load profile), so ``step()`` needs no setpoint.  The profile seeds are the scenario seeds.  This is
        NOT the profile the live runner draws for that scenario seed: its global stream is further along by then, by whatever the
        composer's randomiser drew from it, and that consumption is not restated.  What is reproduced is the runner's profile for
        a stream seeded just before it (np.random.seed(seed) immediately before run_scenario).  ``storage`` as for the constructor
        (a bank of ``bank_seeds`` is built with the same).
        ``episode_streams`` as for the constructor (it needs ``autoreset`` and ``noise_generator="device"``): every episode then begins
        the runner's streams anew -- a restart from bank entry ``s`` the noise of ``RandomState(42)`` and the profile of
        ``RandomState(bank_seeds[s])`` (``bank_noise_seeds=[42] * M``, ``bank_profile_seeds=bank_seeds``), a restart from the plant's own
        snapshot its own -- so each (plant, episode) is bit for bit the run of a fresh ``action_test(action, [that scenario's seed])``.
        ``episode_records`` = a capacity, or True for the default one: ``enable_episode_records(capacity)`` (needs ``autoreset``; a
        summary enabled later is not part of these records -- call ``enable_episode_records`` after ``enable_maintenance_summary`` for that)."""
        if max_episode_steps is not None and not autoreset:
            raise ValueError("max_episode_steps needs autoreset=True")
        if episode_streams:      # refused before any device work
            cls._check_episode_streams(autoreset, True, noise_generator, True, power_profile_steps is not None)
        if episode_records is not None and episode_records is not False and not autoreset:
            raise ValueError("episode_records needs autoreset=True: the records are the episodes the autoreset ends")
        from . import scenarios
        env = cls(len(seeds), dt=dt, heat_source="constant", noise_enabled=True, noise_std_percent=0.1,
                  noise_seeds=[42] * len(seeds), device=device, maintenance=True, params=params, noise_generator=noise_generator,
                  component_maintenance=component_maintenance, component_thresholds=component_thresholds, diagnostics=diagnostics, storage=storage,
                  power_profile=None if power_profile_steps is None else dict(seeds=list(seeds), steps=int(power_profile_steps)))
        eff = float(env.get_field("pump.lubrication_effectiveness")[0].item())
        env.set_fields(scenarios.action_test_fields(action, seeds, eff, randomize=randomize))
        # what a state log of these plants needs beside their state: the composer's provider names and the values the constructor
        # fixed from the initial conditions (nuclear_sim_amd/statelog.py)
        env.log_naming = "composed"
        env.log_side_columns = scenarios.log_side_columns(action, seeds, randomize=randomize)
        if autoreset:
            env.snapshot()
            env._enable_autoreset(max_episode_steps)
        if bank_seeds is not None:
            bank = cls.action_test(action, bank_seeds, dt=dt, device=device, randomize=randomize, params=params,
                                   component_maintenance=component_maintenance, component_thresholds=component_thresholds, diagnostics=diagnostics, storage=storage)
            env.set_start_bank(bank)
            torch.cuda.current_stream(env.device).synchronize()     # the copy has read the bank batch's arena
            bank.close()
        if maintenance_log is not None:
            env.enable_maintenance_log(maintenance_log)
        if episode_streams:      # after the bank: the tables are checked against its entries
            if bank_seeds is None:
                env.enable_episode_streams()
            else:
                env.enable_episode_streams(bank_noise_seeds=[42] * len(bank_seeds),
                                           bank_profile_seeds=None if power_profile_steps is None else list(bank_seeds))
        if episode_records is not None and episode_records is not False:
            env.enable_episode_records(None if episode_records is True else int(episode_records))
        return env

    # ------------------------------------------------------------------ helpers
    def _make_noise(self, seeds):
        """the heat-source noise stream of ``noise_generator``: drawn on the host, or on the device by the handle's generators"""
        if self.noise_generator == "device":
            return DeviceHeatSourceNoise(self, seeds)
        return HeatSourceNoise(seeds, device=self.device)

    def set_step_kernel(self, variant: int) -> None:
        """0 = by batch size (default), 1 = one-wave kernel, 2 = two-wave kernel, 3 = its 256-register build at any size, 4 = the
        one-wave kernel with streaming state stores (what 0 takes above 114 688 plants), 5 = four-wave kernel (what 0 takes up
        to 32 768 plants and between 45 057 and 114 688, where the handle's arena is segmented); same results to the last bit
        or two (include/npb.h)"""
        _lib.check(self.L.npb_set_step_kernel(self._h, int(variant)), self._h)

    def last_step_kernel(self) -> str:
        """the kernel the last step() actually launched, by the name rocprofv3 lists it under ("" before the first step)"""
        return self.L.npb_step_kernel_name(self.L.npb_debug_last_step_kernel(self._h)).decode()

    def enable_diagnostics(self, on: bool = True, carried: bool = False):
        """Have every following step also write the step-internal diagnostics (include/npb.h NPB_DIAG_*: per turbine stage inlet /
        outlet pressure and temperature, power output, loading factor) into ``self.diagnostics`` ([DIAG_DIM, n] on the device,
        rows in _lib.DIAG_STAGE_VALUES order x 14 stages).  The step then runs the diagnostics build of the one-wave kernel at
        every batch size: meant for state logging, not for throughput.

        ``carried=True`` (what the constructor's ``diagnostics=True`` does) also has the handle treat the rows the step carries in
        that buffer (_lib.DIAG_CARRIED_ROWS) as plant state (npb_carry_diagnostics): the next ``snapshot()`` records them, a start bank
        set from a carrying env holds them, ``restore`` / ``restore_from_bank`` / the autoreset put them back per plant and the
        resets reset them, all on the device -- Python no longer touches them -- and ``diagnostics_state()`` checkpoints them.  On an
        env whose diagnostics are already on it keeps the buffer and its values.  With ``carried=False`` the rows are not part of any
        snapshot: ``reset`` / ``restore`` / ``restore_from_bank`` put a freshly constructed plant's values, and autoreset is refused."""
        if on and carried and self._diag_buf is not None:      # the buffer stays: its rows are the plant's
            _lib.check(self.L.npb_carry_diagnostics(self._h, 1), self._h)
            self._diag_carried = True
        elif on:
            pitch = (self.n + 63) // 64 * 64
            buf = torch.zeros((_lib.DIAG_DIM, pitch), dtype=torch.float64, device=self.device)
            for row, value in _lib.DIAG_CARRIED_ROWS.items():
                buf[row].fill_(value)
            _lib.check(self.L.npb_set_diagnostics(self._h, ctypes.c_void_p(buf.data_ptr()), pitch), self._h)
            self._diag_buf = buf
            self.diagnostics = self._diag_buf[:, : self.n]
            if carried:
                if not hasattr(self.L, "npb_carry_diagnostics"):
                    raise _lib.NpbError("libnpb.so has no npb_carry_diagnostics (older than ABI 151): rebuild")
                _lib.check(self.L.npb_carry_diagnostics(self._h, 1), self._h)
            self._diag_carried = bool(carried)
        else:
            _lib.check(self.L.npb_set_diagnostics(self._h, None, 0), self._h)      # (switches the carrying off with it)
            self._diag_buf = None; self.diagnostics = None; self._diag_carried = False
        return self.diagnostics

    def diagnostics_state(self) -> torch.Tensor:
        """[len(_lib.DIAG_CARRIED_ROWS), n] copy of the diagnostics rows the step carries (npb_get_diagnostics_state; rows in
        _lib.DIAG_CARRIED_ROWS order).  Plant state that lives outside the arena: a checkpoint of an env with ``diagnostics=True``
        saves it beside ``state_arrays()``.  Needs the rows carried (``diagnostics=True`` / ``enable_diagnostics(carried=True)``)."""
        t = torch.empty((len(_lib.DIAG_CARRIED_ROWS), self.n), dtype=torch.float64, device=self.device)
        _lib.check(self.L.npb_get_diagnostics_state(self._h, self._p(t), self._stream()), self._h)
        return t

    def load_diagnostics_state(self, state) -> None:
        """the inverse of ``diagnostics_state`` (npb_set_diagnostics_state)"""
        t = torch.as_tensor(state, dtype=torch.float64).to(self.device).contiguous()
        if t.shape != (len(_lib.DIAG_CARRIED_ROWS), self.n):
            raise ValueError("diagnostics state must be [%d, %d]" % (len(_lib.DIAG_CARRIED_ROWS), self.n))
        _lib.check(self.L.npb_set_diagnostics_state(self._h, self._p(t), self._stream()), self._h)

    def _reset_carried_diagnostics(self, mask) -> None:
        """The diagnostics rows the step carries from one step to the next (accumulators, latches, values kept while equipment
        rests: _lib.DIAG_CARRIED_ROWS) back to a freshly constructed plant's, for the masked plants: they are plant state that lives
        in this buffer instead of the arena, so every reset must take them along.  With the rows carried
        (``enable_diagnostics(carried=True)``) the device does that, with what the snapshot or the bank holds: nothing to do here."""
        buf = getattr(self, "_diag_buf", None)
        if buf is None or self._diag_carried:
            return
        for row, value in _lib.DIAG_CARRIED_ROWS.items():
            if mask is None:
                buf[row].fill_(value)
            else:
                buf[row, : self.n].masked_fill_(mask.to(torch.bool), value)

    def enable_maintenance_log(self, capacity: Optional[int] = 65536) -> None:
        """Have every step append the work orders the automatic maintenance creates and completes to a log on the device
        (npb_set_maintenance_log: one record per event, include/npb_maint.h npb_maint_event_t) that ``maintenance_log()`` drains:
        what the reference keeps in WorkOrderManager.work_orders / completed_work_orders and the data-gen runner exports as
        ``*_work_orders.csv`` / ``*_maintenance_actions.csv``.  ``capacity`` records are allocated; events past them are counted,
        not written, until the next drain.  ``None`` turns the log off.  The log is output only: ``snapshot``, ``restore``, the
        autoreset and the start bank neither read nor reset it, so a plant's episodes are told apart by time alone, and after a
        restore its work-order numbers restart from the restored counters, as a fresh reference simulator's would."""
        if capacity is None:      # (without a log there is nothing to fold: the library turns a summary off with it)
            _lib.check(self.L.npb_set_maintenance_log(self._h, None, 0, None), self._h)
            self._mlog = None
            self._msum = None
            return
        if not self.params.maint_enabled:
            raise ValueError("the maintenance log needs the automatic maintenance (maintenance=True)")
        cap = int(capacity)
        if cap < 0:
            raise ValueError("capacity must be >= 0")
        from . import maintlog
        nbytes = int(self.L.npb_maint_event_bytes())
        assert nbytes == maintlog.EVENT_DTYPE.itemsize, (nbytes, maintlog.EVENT_DTYPE.itemsize)
        log = recordlog.allocate(self.device, cap, [("records", (max(cap, 1), nbytes), torch.uint8, 0)])      # (capacity 0 still has a buffer to point at)
        _lib.check(self.L.npb_set_maintenance_log(self._h, self._p(log["dev"]["records"]), cap, self._p(log["cursor"])), self._h)
        self._mlog = log
        ms = self._msum
        if ms is not None:      # a summary that consumed a staging log of its own now folds the caller's log, and leaves it to the caller
            ms["desc"].consume = 0
            ms["words"].zero_()
            _lib.check(self.L.npb_set_maintenance_summary(self._h, ctypes.byref(ms["desc"])), self._h)
            ms["consume"] = False

    def maintenance_log_records(self, clear: bool = True, allow_overflow: bool = False) -> np.ndarray:
        """Drain the log on the env's stream: the records (numpy, ``maintlog.EVENT_DTYPE``) in the device's order.  A log past its
        capacity raises, naming how many events were dropped, and is left as it is, unless ``allow_overflow``."""
        from . import maintlog
        ms = self._msum
        if ms is not None and ms["consume"]:
            raise _lib.NpbError("the maintenance summary consumes the log (enable_maintenance_summary's staging ring): there is nothing to "
                                "drain; enable_maintenance_summary(..., keep_log=True) keeps the records")
        raw = recordlog.drain(self._on("_mlog"), self.device, "maintenance log", "events", "enable_maintenance_log", clear, allow_overflow)
        if clear and ms is not None:      # the summary has folded what was drained: its mark goes back with the cursor
            ms["words"][0].zero_()
        return raw["records"].reshape(-1).view(maintlog.EVENT_DTYPE)

    def maintenance_log(self, clear: bool = True, allow_overflow: bool = False) -> Dict[str, np.ndarray]:
        """``maintenance_log_records`` as columns sorted by (plant, time, completion before creation, pump), named as the
        reference's export (nuclear_sim_amd/maintlog.py): plant, pump, action_type, event_type, timestamp_minutes / _hours,
        work_order_id, component_id, priority, work_order_type, title, created_date, planned_start_date, actual_completion_date,
        bearing, trigger_parameters, has_handler; with ``component_maintenance`` also success (a completed component order's result)."""
        from . import maintlog
        rec = self.maintenance_log_records(clear=clear, allow_overflow=allow_overflow)
        handlers = [int(self.L.npb_maint_action_has_handler(a)) for a in range(len(_lib.MAINT_ACTIONS))]
        return maintlog.columns(rec, _lib.MAINT_ACTIONS, _lib.MAINT_PARAMS, handlers, naming=self.log_naming, with_success=self.component_maintenance)

    def write_maintenance_log(self, path: str, clear: bool = True, allow_overflow: bool = False) -> None:
        """Drain the log into a CSV (``.csv``) or Parquet file"""
        from . import maintlog
        maintlog.write(self.maintenance_log(clear=clear, allow_overflow=allow_overflow), path)

    def enable_maintenance_summary(self, keys, since_minutes: float = 0.0, keep_log: bool = False, operator: bool = False,
                                   log_capacity: Optional[int] = None, include_logged: bool = False) -> None:
        """Have the device fold the maintenance events into a per-plant summary (npb_set_maintenance_summary): per key and plant the time
        the first matching work order was created and the first was completed, and how many were -- what the data-gen runner returns of a
        finished scenario (maintenance_scenario_runner.py:431-468) and what the timing optimiser reads of a probe run
        (timing_optimizer.py:273-320), without draining anything.  ``keys``: up to 16, each a plain action name of the feedwater catalog or
        ``(catalog_name, action_name_or_None, unit_or_None)`` with the catalogs "feedwater", "component", "turbine" (None = any;
        ``_lib.summary_key``).  A key matches the work-order records of its catalog; ``operator=True`` adds the actions a caller ordered
        (``perform_*_maintenance``), which count as completions at the time of the call.  Records before ``since_minutes`` (plant clock) are
        dropped: the runner's tracking_start_hours.  ``None`` for ``keys`` turns the summary off.

        The summary is folded from the event log behind every step and every ``perform_*_maintenance`` call, on the device, with no
        synchronisation.  Without a log of the caller's (``enable_maintenance_log``) it allocates a staging log of ``max(4 * n, 4096)``
        records (``log_capacity`` overrides it; at least n) -- four creations per plant and step -- and consumes it at every fold, so nothing fills up over a long run and
        ``maintenance_log*()`` refuses; with the caller's log, or with ``keep_log=True``, the records stay for the caller to drain.  Events
        that did not fit the log are counted in ``maintenance_summary()["dropped"]``.  ``include_logged=True`` also folds, at once, the
        records the caller's log already holds: an existing log summarised under new keys.  Output only, like the log: ``snapshot``,
        ``restore``, the autoreset and the start bank leave it alone; ``clear_maintenance_summary(mask)`` starts the masked plants afresh."""
        er = self._erec
        if er is not None and (er["n_keys"] or er["desc"].clear_summary):
            raise _lib.NpbError("episode records that copy or clear the maintenance summary are on: disable_episode_records() first")
        # (the task and the features may read the count tables too: they keep the tensors they read alive, and are not refused)
        if self._readers_of(("n_created", "n_completed"), among=("_ewin",)):
            raise _lib.NpbError("event windows with a work_order / completed trigger read the maintenance summary's tables: enable_event_windows(None) first")
        if keys is None:
            if self._msum is not None:
                _lib.check(self.L.npb_set_maintenance_summary(self._h, None), self._h)
                if self._msum["own_log"]:
                    self._msum = None
                    self.enable_maintenance_log(None)
                self._msum = None
            return
        K = [_lib.summary_key(k, operator=operator) for k in keys]      # an unknown name is refused before any device work
        if not 1 <= len(K) <= _lib.SUMMARY_MAX_KEYS:
            raise ValueError("a maintenance summary has 1 to %d keys, not %d" % (_lib.SUMMARY_MAX_KEYS, len(K)))
        if not hasattr(self.L, "npb_set_maintenance_summary"):
            raise _lib.NpbError("libnpb.so has no npb_set_maintenance_summary (older than ABI 154): rebuild")
        prev = self._msum
        own_log = self._mlog is None or (prev is not None and prev["own_log"])
        if own_log:
            self._msum = None
            self.enable_maintenance_log(max(4 * self.n, 4096) if log_capacity is None else int(log_capacity))
        consume = own_log and not keep_log
        with torch.cuda.device(self.device):
            times = torch.full((2, len(K), self.n), float("inf"), dtype=torch.float64, device=self.device)
            counts = torch.zeros((2, len(K), self.n), dtype=torch.int32, device=self.device)
            words = torch.zeros(2, dtype=torch.int32, device=self.device)      # folded, dropped: uint32 on the device
        d = _lib.NpbMaintSummaryDesc()
        d.n_keys, d.consume, d.since_minutes = len(K), int(consume), float(since_minutes)
        for j, (catalog, action, unit, kinds) in enumerate(K):
            d.keys[j].catalog, d.keys[j].action, d.keys[j].unit, d.keys[j].kinds = catalog, action, unit, kinds
        d.first_created, d.first_completed = times[0].data_ptr(), times[1].data_ptr()
        d.n_created, d.n_completed = counts[0].data_ptr(), counts[1].data_ptr()
        d.folded, d.dropped = words[0:].data_ptr(), words[1:].data_ptr()
        if not consume and not include_logged:      # records already in the caller's log are not this summary's: it starts at the cursor
            words[0:1].copy_(self._mlog["cursor"])      # (a cursor past the capacity: the fold starts at the capacity)
        _lib.check(self.L.npb_set_maintenance_summary(self._h, ctypes.byref(d)), self._h)
        self._msum = {"desc": d, "times": times, "counts": counts, "words": words, "keys": K, "consume": consume, "own_log": own_log}
        if include_logged:      # summarise what the caller's log already holds, under these keys, at once
            self.fold_maintenance_summary()

    def maintenance_summary(self) -> Dict[str, torch.Tensor]:
        """The summary's tables, [n_keys, n] each, on the device: ``first_created`` / ``first_completed`` (plant minutes, float64, +inf =
        never), ``n_created`` / ``n_completed`` (int32), and ``dropped`` (a 0-d int32 tensor: events the log had no room for, which the
        summary therefore never saw).  The env's own buffers, as ``info`` is: current after every ``step`` and ``perform_*_maintenance``,
        valid in stream order, never synchronised here."""
        ms = self._on("_msum")
        return {"first_created": ms["times"][0], "first_completed": ms["times"][1], "n_created": ms["counts"][0],
                "n_completed": ms["counts"][1], "dropped": ms["words"][1]}

    def clear_maintenance_summary(self, mask=None) -> None:
        """the summary rows of the masked plants (None = all) back to "never" and 0 (npb_maint_summary_clear): what a caller does for the
        plants it restarted when it wants per-episode summaries"""
        self._clear("_msum", self.L.npb_maint_summary_clear, mask)

    def fold_maintenance_summary(self) -> None:
        """fold the log into the summary now (npb_maint_summary_fold); ``step`` and the ``perform_*_maintenance`` calls do it themselves"""
        self._on("_msum")
        _lib.check(self.L.npb_maint_summary_fold(self._h, self._stream()), self._h)

    def enable_episode_records(self, capacity: Optional[int] = None, final_obs: bool = False, summary: Optional[bool] = None,
                               clear_summary: Optional[bool] = None, *, off: bool = False, stats: Optional[bool] = None,
                               clear_stats: Optional[bool] = None) -> None:
        """Have the device keep a log of FINISHED episodes (npb_set_episode_records): behind every step, one record per plant whose episode
        ended on it -- plant, episode index, bank entry it started from, length, return, terminated / truncated, the step's trip flags, the
        step number, the plant clock, with ``final_obs`` the terminal observation and with ``summary`` that episode's rows of the work-order
        summary -- which ``episode_records()`` drains whenever the caller chooses.  Needs autoreset.  ``capacity`` records are allocated
        (None = ``max(4 * n, 4096)``); episodes past them are counted, not written, until the next drain.  ``summary`` and
        ``clear_summary`` default to whether a maintenance summary is enabled; ``clear_summary`` puts an ended plant's summary rows back to
        "never" / 0 on the device, so that every record holds the work orders of its own episode (off, the summary goes on counting across
        restarts, as it does without records).  ``stats`` and ``clear_stats`` default to whether column statistics are enabled
        (``enable_column_stats``): with ``stats`` every record carries the plant's cells of each table kept as of the terminal step
        (``stat_min`` ... [m, n_cols] and ``stat_n_samples``), and ``clear_stats`` puts an ended plant's cells back to the empty values,
        so that each record holds the statistics of its own episode and ``stat_n_samples == length``.  ``off=True`` turns the records off
        and releases the buffers.  An episode the caller abandons (``restore``, ``restore_from_bank``, ``reset``) starts the next index
        and leaves no record."""
        if off:
            if self._erec is not None:
                _lib.check(self.L.npb_set_episode_records(self._h, None), self._h)
            self._erec = None
            return
        if not hasattr(self.L, "npb_set_episode_records"):
            raise _lib.NpbError("libnpb.so has no npb_set_episode_records: rebuild")
        if self._episode is None:
            raise ValueError("episode records need autoreset=True: they are the episodes the autoreset ends")
        has_summary = self._msum is not None
        summary = has_summary if summary is None else bool(summary)
        clear_summary = has_summary if clear_summary is None else bool(clear_summary)
        if (summary or clear_summary) and not has_summary:
            raise ValueError("episode records with summary / clear_summary need enable_maintenance_summary() first")
        cst = self._cstats
        stats = (cst is not None) if stats is None else bool(stats)
        clear_stats = (cst is not None) if clear_stats is None else bool(clear_stats)
        if (stats or clear_stats) and cst is None:
            raise ValueError("episode records with stats / clear_stats need enable_column_stats() first")
        cap = max(4 * self.n, 4096) if capacity is None else int(capacity)
        if cap < 1:
            raise ValueError("capacity must be >= 1")
        n_keys = len(self._msum["keys"]) if summary else 0
        d = _lib.NpbEpisodeRecordsDesc()
        d.capacity, d.clear_summary = cap, int(clear_summary)
        log = recordlog.allocate(self.device, cap)

        def column(name, shape, dtype, slot_axis=0, desc=d, member=None):      # (a table's records lie along its last axis)
            setattr(desc, member or name, recordlog.add_column(log, name, shape, dtype, slot_axis).data_ptr())
        for name, np_type in _lib.EPISODE_RECORD_COLUMNS:      # (uint32 trip flags travel as int32 bits)
            column(name, (cap,), torch.float64 if np_type is np.float64 else torch.int32)
        if final_obs:
            column("final_obs", (cap, 22), torch.float64)
        if summary:
            for name in ("first_created", "first_completed"):
                column(name, (n_keys, cap), torch.float64, -1)
            for name in ("n_created", "n_completed"):
                column(name, (n_keys, cap), torch.int32, -1)
        rs = None
        if stats or clear_stats:      # the record-side columns of the statistics, as "stat_<name>"
            rs = _lib.NpbEpisodeRecordStatsDesc()
            rs.clear = int(clear_stats)
            if stats:
                for name in cst["stats"] + ("n_samples",):
                    int_table, per_column = name in ("n_beyond", "n_samples"), name != "n_samples"
                    column("stat_" + name, (len(cst["order"]), cap) if per_column else (cap,), torch.int32 if int_table else torch.float64,
                           -1 if per_column else 0, desc=rs, member=name)
        d.cursor = log["cursor"].data_ptr()
        _lib.check(self.L.npb_set_episode_records(self._h, ctypes.byref(d)), self._h)
        self._erec = None      # (new record columns: the handle has dropped the statistics columns of the old ones with them)
        if rs is None:
            if hasattr(self.L, "npb_set_episode_record_stats"):
                _lib.check(self.L.npb_set_episode_record_stats(self._h, None), self._h)
        else:
            try:
                _lib.check(self.L.npb_set_episode_record_stats(self._h, ctypes.byref(rs)), self._h)
            except _lib.NpbError:
                self.L.npb_set_episode_records(self._h, None)
                raise
        self._erec = dict(log, desc=d, n_keys=n_keys, stats=rs, stat_order=list(cst["order"]) if stats else None)
        self._record_task_cause()

    def _record_task_cause(self) -> None:
        """while records and a task are both on every record carries the task's cause word (npb_set_episode_record_task); the handle drops
        the column with every new set of record columns, so this follows ``enable_episode_records`` and ``set_task``"""
        er = self._erec
        if er is None or self._task is None:
            return
        if "cause" not in er["dev"]:
            recordlog.add_column(er, "cause", (er["capacity"],), torch.int32)      # (uint32 bits travel as int32)
        _lib.check(self.L.npb_set_episode_record_task(self._h, self._p(er["dev"]["cause"])), self._h)

    def _drop_record_task_cause(self) -> None:
        """the records without the cause column (the handle refuses another task, or none, while they hold the old one's)"""
        er = self._erec
        if er is not None and "cause" in er["dev"]:
            _lib.check(self.L.npb_set_episode_record_task(self._h, None), self._h)
            recordlog.drop_column(er, "cause")

    def disable_episode_records(self) -> None:
        """episode records off; the buffers are released"""
        self.enable_episode_records(off=True)

    def episode_records(self, clear: bool = True, allow_overflow: bool = False) -> Dict[str, np.ndarray]:
        """Drain the episode records on the env's stream: numpy columns of m records sorted by (step, plant) -- ``plant``, ``episode``,
        ``start`` (-1 = not from the bank), ``length``, ``flags``, ``terminated`` / ``truncated`` (bool), ``trip_flags`` (uint32), ``step``
        (steps since the records were enabled, 0 = the first), ``ret``, ``end_time`` (plant minutes); with ``final_obs``
        ``final_observation`` [m, 22]; with ``summary`` ``first_created`` / ``first_completed`` (float64, +inf = never) and ``n_created`` /
        ``n_completed`` (int32), [m, n_keys]; with ``stats`` ``stat_min`` ... (the tables ``enable_column_stats`` keeps) [m, n_cols] and
        ``stat_n_samples``; while a task is set (``set_task``) ``cause`` (uint32: the rules that ended the episode, 0 = none did).  A
        log past its capacity raises, naming how many episodes were dropped, and is left as it is,
        unless ``allow_overflow`` (which of one step's episodes fitted is then not defined)."""
        er = self._on("_erec")
        raw = recordlog.drain(er, self.device, "episode records", "episodes", "enable_episode_records", clear, allow_overflow)
        order = np.lexsort((raw["plant"], raw["step"]))
        out = {name: raw[name][order] for name, _ in _lib.EPISODE_RECORD_COLUMNS}
        out["trip_flags"] = out["trip_flags"].view(np.uint32)
        out["terminated"], out["truncated"] = (out["flags"] & 1) != 0, (out["flags"] & 2) != 0
        if "final_obs" in raw:
            out["final_observation"] = raw["final_obs"][order]
        if "cause" in raw:
            out["cause"] = np.ascontiguousarray(raw["cause"][order]).view(np.uint32)
        for name in ("first_created", "first_completed", "n_created", "n_completed"):
            if name in raw:
                out[name] = np.ascontiguousarray(raw[name][order])
        for name in raw:      # the episode's column statistics, [m, n_cols] in the caller's column order
            if name.startswith("stat_"):
                a = raw[name][order]
                out[name] = np.ascontiguousarray(a if a.ndim == 1 else a[:, er["stat_order"]])
        return out

    def write_episode_records(self, path: str, clear: bool = True, allow_overflow: bool = False) -> None:
        """Drain the episode records into a CSV (``.csv``) or Parquet file: one row per episode; the terminal observation as
        ``final_observation_0`` .. ``_21``, the summary tables as ``first_created_0`` .. per key and the column statistics as
        ``stat_min_0`` .. per column"""
        from . import maintlog
        cols = {}
        for name, a in self.episode_records(clear=clear, allow_overflow=allow_overflow).items():
            if a.ndim == 1:
                cols[name] = a
            else:
                cols.update({"%s_%d" % (name, j): np.ascontiguousarray(a[:, j]) for j in range(a.shape[1])})
        maintlog.write(cols, path)

    def _side_buffers(self) -> dict:
        """THE buffers a per-plant column's side source may point into, by the names ``_lib.column_word`` gives them: the step's outputs,
        the summary's two count tables while a summary is on, the task's reward and cause while a task is on.  Which of them a feature
        accepts is decided by its vocabulary in ``_lib``, not by what is listed here"""
        buffers = {"info": self._info_buf, "obs": self._obs, "reward": self._reward, "flags": self._flags, "done": self._done}
        ms, tk, ct = self._msum, self._task, self._ctl
        if ms is not None:
            buffers.update(n_created=ms["counts"][0], n_completed=ms["counts"][1])
        if tk is not None:
            buffers.update(task_reward=tk["reward"], task_cause=tk["cause"])
        if ct is not None:
            buffers.update(control=ct["held"], control_prev=ct["prev"])
        if self._ord is not None:
            buffers.update(order=self._ord["fired"])
        return buffers

    # ------------------------------------------------------------------ what the attachments share
    # The per-step attachments -- maintenance log and summary, episode records, column statistics, event windows, task, features,
    # controls, rollout: None = off, else what the enable_* / set_* method keeps of it.  __init__ sets them; the class has them too, so that a
    # refusal "before any device work" can be checked on an object made without it.  ``_on`` reads them, with these refusals:
    _mlog = _msum = _erec = _cstats = _ewin = _task = _feat = _ctl = _ord = _roll = _norm = _pol = None
    _max_episode_steps = 0      # the autoreset's limit, 0 = none (``_enable_autoreset``)
    _OFF = {"_mlog": "no maintenance log: enable_maintenance_log() first", "_msum": "no maintenance summary: enable_maintenance_summary() first",
            "_erec": "no episode records: enable_episode_records() first", "_cstats": "no column statistics: enable_column_stats() first",
            "_ewin": "no event windows: enable_event_windows() first", "_task": "no task: set_task() first",
            "_feat": "no features: set_features() first", "_ctl": "no controls: set_controls() first",
            "_ord": "no order rules: set_control_orders() first", "_roll": "no rollout: set_rollout() first",
            "_norm": "no normaliser: set_normalizer() first", "_pol": "no policy: set_policy() first"}
    # who reads side buffers, as a refusal names them: each keeps ``"reads"``, the buffers its request resolved to (``_reading``)
    _CONSUMERS = {"_task": "the task", "_feat": "the features", "_cstats": "the column statistics", "_ewin": "the event windows",
                  "_norm": "the normaliser"}

    def _on(self, attr) -> dict:
        """THE "is it on" of an attachment: what it keeps, or its refusal"""
        what = getattr(self, attr)
        if what is None:
            raise _lib.NpbError(self._OFF[attr])
        return what

    def _clear(self, attr, clear, mask) -> dict:
        """the body of the ``clear_*`` methods: the attachment must be on, the mask (None = all) goes to the library's ``clear`` as a column"""
        what = self._on(attr)
        _lib.check(clear(self._h, self._p(self._col(mask, torch.uint8)), self._stream()), self._h)
        return what

    @staticmethod
    def _reading(req, buffers) -> dict:
        """What a consumer keeps of the side buffers its request resolved to -- columns, reference columns and triggers alike:
        ``"reads"``, the frozenset of their names, by which ``_readers_of`` finds it, and ``"holds"``, the tensors themselves, so that
        none is freed while a kernel reads it, whether or not its provider refuses to change meanwhile"""
        rows = list(req.get("columns", ())) + list(req.get("triggers", ()))
        reads = frozenset([side[0] for side in req.get("sides", ())] + [R["side"][0] for R in rows if R["side"]])
        return {"reads": reads, "holds": [buffers[name] for name in sorted(reads)]}

    def _readers_of(self, names, among=tuple(_CONSUMERS)):
        """the consumers, of ``among`` and in its order, that read any of the side buffers ``names``, as a refusal names them"""
        return [self._CONSUMERS[attr] for attr in among if getattr(self, attr) is not None and getattr(self, attr)["reads"] & set(names)]

    def _n_controls(self) -> int:
        """the axis count while controls are set, else 0: what ``_lib.column_word`` takes as ``controls``"""
        return 0 if self._ctl is None else self._ctl["held"].shape[0]

    def _n_orders(self) -> int:
        """the rule count while order rules are set, else 0: what ``_lib.column_word`` takes as ``orders``"""
        return 0 if self._ord is None else self._ord["fired"].shape[0]

    def _get_state(self, attr, getter) -> Dict[str, np.ndarray]:
        """an attachment's checkpointed state, the arrays of its ``"state"`` tuple of (name, dtype, shape) filled by the library's
        ``getter``, which takes them in that order (an empty one as NULL)"""
        out = {name: np.zeros(shape, dtype=dtype) for name, dtype, shape in self._on(attr)["state"]}
        _lib.check(getter(self._h, *[a.ctypes.data if a.size else None for a in out.values()], self._stream()), self._h)
        return out

    def _load_state(self, attr, setter, state) -> list:
        """the inverse: ``state``'s entries coerced to the dtypes and shapes of the ``"state"`` tuple and handed to the library's ``setter``"""
        parts = [np.ascontiguousarray(np.asarray(state[name], dtype=dtype).reshape(shape)) for name, dtype, shape in self._on(attr)["state"]]
        _lib.check(setter(self._h, *[a.ctypes.data if a.size else None for a in parts], self._stream()), self._h)
        return parts

    def _column_samples(self, columns) -> torch.Tensor:
        """the rows ``columns`` (``_lib.column_word``'s answers) name as they are NOW, widened to float64, [len(columns), n] on the device"""
        buffers = self._side_buffers()
        rows = []
        for C in columns:
            if C["member"] is not None:
                rows.append(self._get_slot("f64" if C["member"][0] == 0 else "i32", C["member"][1]).to(torch.float64))
            else:
                name, offset, stride, _kind = C["side"]
                rows.append(buffers[name].reshape(-1)[self._side_first(name, offset)::stride][:self.n].to(torch.float64))
        return torch.stack(rows)

    def _side_first(self, name, offset) -> int:
        """the element of side buffer ``name`` that holds plant 0's value of the column at ``offset``: a summary table is [n_keys][n], the
        controls' held and previous values [n_axes][n], the order rules' fired [n_orders][n]"""
        return offset * self.n if name in ("n_created", "n_completed", "control", "control_prev", "order") else offset

    def _fill_source(self, S, buffers, name, offset, stride, kind="f64") -> None:
        """fill the NpbSampleSource ``S`` from a side column as ``_lib.column_word`` names it: one value per plant"""
        S.base = buffers[name].data_ptr() + {"f64": 8, "i32": 4, "u8": 1}[kind] * self._side_first(name, offset)
        S.type, S.rows, S.row_stride, S.plant_stride = _lib.SAMPLE_TYPES[kind], 1, 0, stride

    def _fill_column(self, C, buffers, where) -> None:
        """fill the {from_source, kind, slot, source} head of an NpbEventTrigger or NpbTaskColumn from ``_lib.column_word``'s answer"""
        if where["member"] is not None:
            C.from_source, (C.kind, C.slot) = 0, where["member"]
        else:
            C.from_source = 1
            self._fill_source(C.source, buffers, *where["side"])

    def _fill_columns(self, d, req, buffers):
        """fill n_fields / kinds / slots / n_sources / sources of the descriptor ``d`` from a request's members and sides; returns the ctypes
        arrays, which the caller keeps alive for as long as the descriptor is read"""
        nm, ns = len(req["members"]), len(req["sides"])
        kinds = (ctypes.c_int * max(nm, 1))(*[m[0] for m in req["members"]])
        slots = (ctypes.c_int * max(nm, 1))(*[m[1] for m in req["members"]])
        side = (_lib.NpbSampleSource * max(ns, 1))()
        for k, where in enumerate(req["sides"]):
            self._fill_source(side[k], buffers, *where)
        d.n_fields, d.kinds, d.slots, d.n_sources, d.sources = nm, kinds, slots, ns, side
        return kinds, slots, side

    def enable_column_stats(self, columns, limits=None, stats=("min", "max", "sum", "sumsq", "last")) -> None:
        """Have the device fold per-plant statistics of ``columns`` behind every step (npb_set_column_stats): one more launch, a thread per
        (column, plant), the sample being the end-of-step state of the episode the step belonged to, before any restore.  ``columns``: up
        to 32, each a state member as ``set_fields`` keys it (``name``, ``(name, instance)`` or ``(name, instance, k)``), ``("info",
        column_name)``, ``("obs", i)``, ``"reward"`` or, while a task is set (``set_task``), ``"task_reward"``.  ``limits``:
        ``{column_index: (">" | "<", value)}``; ``stats``: the tables to keep,
        of "min", "max", "sum", "sumsq", "last" and, for columns with a limit, "first_beyond" (the plant clock after the first step whose
        sample was beyond the limit, +inf = never) and "n_beyond" (samples beyond it).  ``nuclear_sim_amd.colstats.fold`` is the same in
        numpy, bit for bit.  ``None`` for ``columns`` turns it off.  Output only, like the maintenance summary: ``snapshot``, ``restore``,
        the resets, the autoreset and the start bank leave the tables alone; ``clear_column_stats(mask)`` starts the masked plants afresh,
        and episode records enabled afterwards do so for every episode that ends (``enable_episode_records(stats=..., clear_stats=...)``)."""
        if self._erec is not None and self._erec.get("stats") is not None:
            raise _lib.NpbError("episode records that copy or clear the column statistics are on: disable_episode_records() first")
        if columns is None:
            if self._cstats is not None:
                _lib.check(self.L.npb_set_column_stats(self._h, None), self._h)
            self._cstats = None
            return
        req = _lib.column_stats_request(columns, limits, stats, INFO_COLUMNS, self._task is not None, self._n_controls(), self._n_orders())      # an unknown name, index or statistic is refused here
        if not hasattr(self.L, "npb_set_column_stats"):
            raise _lib.NpbError("libnpb.so has no npb_set_column_stats: rebuild")
        n_cols = len(req["members"]) + len(req["sides"])
        d = _lib.NpbColumnStatsDesc()
        buffers = self._side_buffers()
        keep = self._fill_columns(d, req, buffers)      # (the library copies the descriptor's arrays during the call)
        d.direction, d.limit = (ctypes.c_int * n_cols)(*req["direction"]), (ctypes.c_double * n_cols)(*req["limit"])
        from . import colstats
        tables = {}
        with torch.cuda.device(self.device):
            for name in req["stats"]:
                tables[name] = torch.full((n_cols, self.n), colstats.EMPTY[name], dtype=torch.int32 if name == "n_beyond" else torch.float64,
                                          device=self.device)
                setattr(d, name, tables[name].data_ptr())
            tables["n_samples"] = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        d.n_samples = tables["n_samples"].data_ptr()
        _lib.check(self.L.npb_set_column_stats(self._h, ctypes.byref(d)), self._h)
        self._cstats = dict(self._reading(req, buffers), tables=tables, stats=req["stats"], order=req["order"], columns=list(columns))

    def column_stats(self) -> Dict[str, torch.Tensor]:
        """The statistics' tables, [n_cols, n] each in the order of ``columns``, and ``n_samples`` [n], on the device, never synchronised
        here.  Where ``columns`` lists every state member ahead of every info / obs / reward column -- the order the device keeps them in
        -- these are the env's own buffers, as ``maintenance_summary()``'s are: current after every later ``step`` too.  For a request in
        any other order the tables are an indexed COPY made now, in stream order: it does not follow later steps; call again."""
        cs = self._on("_cstats")
        identity = cs["order"] == list(range(len(cs["order"])))
        return {name: t if (identity or t.dim() == 1) else t[cs["order"]] for name, t in cs["tables"].items()}

    def clear_column_stats(self, mask=None) -> None:
        """the cells of the masked plants (None = all) back to the empty values in every table (npb_column_stats_clear)"""
        self._clear("_cstats", self.L.npb_column_stats_clear, mask)

    def fold_column_stats(self) -> None:
        """fold one sample of the current state now (npb_column_stats_fold); ``step`` does it itself"""
        self._on("_cstats")
        _lib.check(self.L.npb_column_stats_fold(self._h, self._stream()), self._h)

    def enable_event_windows(self, columns, triggers=None, pre: int = 8, post: int = 8, capacity: Optional[int] = None) -> None:
        """Have the device capture a window of ``columns`` around every event (npb_set_event_windows): each plant keeps its last
        ``pre + 1 + post`` end-of-step samples in a ring on the device; a trigger arms a capture, and ``post`` steps later the window --
        ``pre`` samples before the trigger, the trigger sample, ``post`` after -- goes into a record that ``event_windows()`` drains
        whenever the caller chooses.  One more launch behind every step, nothing read back.  ``columns``: 1 to 16, keyed as
        ``enable_column_stats`` keys them.  ``triggers``: 1 to 8, each ``("trip", mask)`` (rising bits of the step's trip flags),
        ``("done",)``, ``("work_order", key_index)`` / ``("completed", key_index)`` (a new work order / completion under that key of
        ``enable_maintenance_summary``, which must be on), ``("maintenance",)`` (the event count goes up), ``(column, ">" | "<",
        value)`` (the edge of a limit) or, while a task is set (``set_task``), ``("task", mask)`` (rising bits of the task's cause column;
        ``"task_reward"`` is then a column too).  ``capacity`` records are allocated (None = ``max(n, 4096)``); captures past them are counted,
        not written, until the next drain.  A capture whose episode ends before ``post`` more steps is taken at once (``early``); a
        restart (autoreset, ``restore``, ``reset``; without autoreset ``clear_event_windows(mask)``) empties the plant's ring and drops an
        armed capture.  ``nuclear_sim_amd.eventwin.record`` is the same in numpy, bit for bit.  ``None`` for ``columns`` turns it off.
        Output only: ``snapshot``, ``restore`` and the start bank leave it alone.  While it is on, the maintenance summary a
        ``work_order`` trigger reads must stay as it is."""
        if columns is None:
            if self._ewin is not None:
                _lib.check(self.L.npb_set_event_windows(self._h, None), self._h)
            self._ewin = None
            return
        ms = self._msum
        req = _lib.event_windows_request(columns, triggers or (), pre, post, INFO_COLUMNS, 0 if ms is None else len(ms["keys"]), self._task is not None,
                                         self._n_controls(), self._n_orders())
        if not hasattr(self.L, "npb_set_event_windows"):
            raise _lib.NpbError("libnpb.so has no npb_set_event_windows: rebuild")
        cap = max(self.n, 4096) if capacity is None else int(capacity)
        if cap < 1:
            raise ValueError("capacity must be >= 1")
        nt = len(req["triggers"])
        n_cols, H = len(req["members"]) + len(req["sides"]), req["pre"] + 1 + req["post"]
        d = _lib.NpbEventWindowsDesc()
        buffers = self._side_buffers()
        keep = self._fill_columns(d, req, buffers)
        trig = (_lib.NpbEventTrigger * nt)()
        for k, T in enumerate(req["triggers"]):
            self._fill_column(trig[k], buffers, T)
            trig[k].mode, trig[k].mask, trig[k].direction, trig[k].limit = _lib.TRIGGER_MODES[T["mode"]], T["mask"], T["direction"], T["limit"]
        d.n_triggers, d.triggers = nt, trig
        d.pre, d.post, d.capacity = req["pre"], req["post"], cap
        shapes = [(name, (cap,), torch.int32, 0) for name in _lib.EVENT_WINDOW_WORDS + ("fired",)]      # (the uint32 fired set travels as int32 bits)
        shapes += [("time", (cap,), torch.float64, 0), ("times", (cap, H), torch.float64, 0), ("values", (cap, H, n_cols), torch.float64, 0)]
        log = recordlog.allocate(self.device, cap, shapes)
        for name, t in log["dev"].items():
            setattr(d, name, t.data_ptr())
        d.cursor = log["cursor"].data_ptr()
        _lib.check(self.L.npb_set_event_windows(self._h, ctypes.byref(d)), self._h)
        self._ewin = dict(self._reading(req, buffers), **log, desc=d, keep=keep + (trig,), order=req["order"],
                          columns=list(columns), pre=req["pre"], post=req["post"], triggers=req["numpy"],
                          bytes=int(self.L.npb_event_windows_bytes(ctypes.byref(d), self.n)))

    def event_windows(self, clear: bool = True, allow_overflow: bool = False) -> Dict[str, np.ndarray]:
        """Drain the event windows on the env's stream, one read-back: numpy columns of m records sorted by (capture step, plant) --
        ``plant``, ``episode``, ``trigger`` (the lowest trigger that fired), ``step`` (the trigger's step since the windows were enabled,
        0 = the first), ``n_pre``, ``n_post``, ``flags``, ``retriggers`` (int32), ``fired`` (uint32: every trigger that fired on that
        step), ``time`` (the plant clock at the trigger), ``times`` [m, H], ``values`` [m, H, n_cols] in the order of ``columns`` (row
        ``pre`` is the trigger sample; rows outside ``[pre - n_pre, pre + n_post]`` are NaN) and ``early`` = ``flags & 1``.  A
        log past its capacity raises, naming how many captures were dropped, and is left as it is, unless ``allow_overflow`` (which of one
        step's captures fitted is then not defined)."""
        ew = self._on("_ewin")
        raw = recordlog.drain(ew, self.device, "event windows", "captures", "enable_event_windows", clear, allow_overflow)
        order = np.lexsort((raw["plant"], raw["step"] + raw["n_post"]))
        out = {name: np.ascontiguousarray(a[order]) for name, a in raw.items()}
        out["fired"] = out["fired"].view(np.uint32)
        out["values"] = np.ascontiguousarray(out["values"][:, :, ew["order"]])
        out["early"] = (out["flags"] & 1) != 0
        return out

    def write_event_windows(self, path: str, clear: bool = True, allow_overflow: bool = False) -> None:
        """Drain the event windows into a CSV (``.csv``) or Parquet file: one row per capture; the clock of row offset k (-pre .. post)
        as ``time_m<k>`` / ``time_p<k>`` and recorded column c at that offset as ``c<c>_m<k>`` / ``c<c>_p<k>``"""
        from . import maintlog
        rec = self.event_windows(clear=clear, allow_overflow=allow_overflow)
        pre = self._ewin["pre"]
        cols = {name: a for name, a in rec.items() if a.ndim == 1}
        for k in range(rec["times"].shape[1]):
            tag = "m%d" % (pre - k) if k < pre else "p%d" % (k - pre)
            cols["time_" + tag] = np.ascontiguousarray(rec["times"][:, k])
            for c in range(rec["values"].shape[2]):
                cols["c%d_%s" % (c, tag)] = np.ascontiguousarray(rec["values"][:, k, c])
        maintlog.write(cols, path)

    def clear_event_windows(self, mask=None) -> None:
        """the masked plants (None = all) unprimed, their rings empty, an armed capture dropped without a record
        (npb_event_windows_clear): what a caller without autoreset does for the plants it restarted"""
        self._clear("_ewin", self.L.npb_event_windows_clear, mask)

    def _task_readers(self):
        """what reads the task's output columns, as a refusal names them"""
        return self._readers_of(("task_reward", "task_cause"), among=("_cstats", "_ewin", "_feat", "_norm"))

    def set_task(self, reward=(), terminate=(), bias: float = 0.0, keep_terms: bool = False) -> None:
        """Define the reward and the termination rule on the device (npb_set_task): behind every step one more launch forms a per-plant
        task reward, a termination flag and a cause word from the end-of-step state and the step's outputs, and everything that deals
        with episodes -- the same-step autoreset, ``info["episode_return"]``, the episode records, the event windows' ``early`` captures
        -- uses them in place of the reference's reward and scram pulse.  Nothing is read back.
        ``reward``: 0 to 16 terms, ``(column, weight)`` or ``(column, weight, kind, ...)`` with kind ``"value"``, ``"abs_err", ref``,
        ``"sq_err", ref`` (ref a number or a second column), ``"beyond", ">" | "<", limit``, ``"excess", ">" | "<", limit``, ``"bits",
        mask`` (an integer column) or ``"delta"`` (this sample minus the plant's previous one; 0 on the first sample of an episode): the
        reward is ``bias + w_0 * f_0 + w_1 * f_1 + ...``.  Columns are keyed as ``enable_column_stats`` keys them (``"reward"`` is the
        step's own reward, so "the reference's reward plus extras" is one ``("reward", 1.0)`` term), or are one of the integer sides
        ``"flags"``, ``"done"``, ``("work_order", key_index)`` / ``("completed", key_index)`` (``enable_maintenance_summary`` first, and
        it must then stay as it is) and ``"maintenance"`` (the event count).
        ``terminate``: 0 to 8 rules, ``("done",)`` (the reference's scram pulse), ``("trip", mask)``, ``(column, ">" | "<", value)`` or
        ``(column, "nonfinite")``, each with an optional trailing terminal reward, added when the rule fires.  Rules are levels: with
        autoreset the plant restarts on that step; without it a level keeps reporting for as long as it holds.  A task without
        ``("done",)`` no longer ends episodes on a scram.
        With a task on ``step()`` returns the task's reward and done, and adds ``info["reference_reward"]``, ``info["task_cause"]``
        (uint32 bits as int32: bit r = rule r fired) and, with ``keep_terms``, ``info["task_terms"]`` [n_terms, n] (each term's w * f);
        ``info["scram_activated"]`` stays the step's column.  ``episode_records()`` gains ``cause``.  ``nuclear_sim_amd.task.evaluate``
        is the same in numpy, bit for bit.  ``set_task(None)`` turns it off; while column statistics or event windows read
        ``"task_reward"`` / ``("task", mask)`` that, and a new task, are refused: turn them off first."""
        if reward is None and not terminate:
            if self._task is None:
                return
            for what in self._task_readers():
                raise _lib.NpbError("set_task(None): %s read 'task_reward' / ('task', mask): turn them off first" % what)
            self._drop_record_task_cause()
            _lib.check(self.L.npb_set_task(self._h, None), self._h)
            self._task = None
            return
        ms = self._msum
        req = _lib.task_request(reward, terminate, bias, INFO_COLUMNS, 0 if ms is None else len(ms["keys"]), self._n_controls(), self._n_orders())      # a bad word is refused here
        if not hasattr(self.L, "npb_set_task"):
            raise _lib.NpbError("libnpb.so has no npb_set_task: rebuild")
        for what in self._task_readers():      # (they hold the old task's output columns)
            raise _lib.NpbError("set_task: %s read 'task_reward' / ('task', mask) of the task that is set: turn them off first" % what)
        buffers = self._side_buffers()
        nt, nr = len(req["terms"]), len(req["rules"])
        terms, rules = (_lib.NpbTaskTerm * max(nt, 1))(), (_lib.NpbTaskRule * max(nr, 1))()
        for k, T in enumerate(req["terms"]):
            self._fill_column(terms[k].column, buffers, req["columns"][T["col"]])
            terms[k].weight, terms[k].kind = T["weight"], _lib.TASK_KINDS[T["kind"]]
            if isinstance(T["ref"], tuple):
                terms[k].ref_from_column = 1
                self._fill_column(terms[k].ref_column, buffers, req["columns"][T["ref"][1]])
            else:
                terms[k].ref = T["ref"]
            terms[k].direction, terms[k].limit, terms[k].mask = T["direction"], T["limit"], T["mask"]
        for k, R in enumerate(req["rules"]):
            self._fill_column(rules[k].column, buffers, req["columns"][R["col"]])
            rules[k].mode, rules[k].mask, rules[k].direction, rules[k].limit = _lib.TASK_MODES[R["mode"]], R["mask"], R["direction"], R["limit"]
            rules[k].terminal_reward = R["terminal_reward"]
        d = _lib.NpbTaskDesc()
        d.n_terms, d.terms, d.n_rules, d.rules, d.bias = nt, terms, nr, rules, req["bias"]
        with torch.cuda.device(self.device):
            out = {"reward": torch.zeros(self.n, dtype=torch.float64, device=self.device),
                   "done": torch.zeros(self.n, dtype=torch.uint8, device=self.device),
                   "cause": torch.zeros(self.n, dtype=torch.int32, device=self.device),      # a uint32 on the device
                   "terms": torch.zeros((nt, self.n), dtype=torch.float64, device=self.device) if keep_terms and nt else None}
        d.reward, d.done, d.cause = out["reward"].data_ptr(), out["done"].data_ptr(), out["cause"].data_ptr()
        d.terms_out = None if out["terms"] is None else out["terms"].data_ptr()
        self._drop_record_task_cause()
        try:
            _lib.check(self.L.npb_set_task(self._h, ctypes.byref(d)), self._h)
        except _lib.NpbError:
            self._record_task_cause()      # (what was set before stays, its cause column in the records too)
            raise
        nd = sum(T["kind"] == "delta" for T in req["terms"])
        self._task = dict(out, **self._reading(req, buffers), request=req,
                          state=(("prev", np.float64, (nd, self.n)), ("primed", np.int32, (self.n,)), ("seen", np.int32, (self.n,))))
        self._record_task_cause()

    def task_spec(self) -> dict:
        """the task as ``nuclear_sim_amd.task.evaluate`` takes it -- {"bias", "terms", "rules"} over the rows of ``task_samples()``"""
        req = self._on("_task")["request"]
        return {"bias": req["bias"], "terms": req["terms"], "rules": req["rules"]}

    def task_samples(self) -> torch.Tensor:
        """The columns the task reads as they are NOW, widened to float64, [n_cols, n] on the device (gather launches and copies: for
        checks and debugging, not for the hot path).  Behind a ``step()`` without autoreset these are the samples the task was formed
        from; a plant the autoreset restarted shows its start state."""
        return self._column_samples(self._on("_task")["request"]["columns"])

    def clear_task(self, mask=None) -> None:
        """the masked plants (None = all) unprimed: their next ``"delta"`` samples are 0 (npb_task_clear) -- what a caller without
        autoreset does for the plants it restarted"""
        self._clear("_task", self.L.npb_task_clear, mask)

    def task_state(self) -> Dict[str, np.ndarray]:
        """The task's own state for a checkpoint (npb_task_get_state), beside ``state_arrays()``: ``prev`` float64 [n_delta, n] (the
        previous samples of the ``"delta"`` terms, in term order), ``primed`` and ``seen`` int32 [n] (the plant has a previous sample;
        the episode index last seen)."""
        return self._get_state("_task", self.L.npb_task_get_state)

    def load_task_state(self, state) -> None:
        """put back what ``task_state()`` returned (npb_task_set_state): the task must be the one it was taken under"""
        want, got = self._on("_task")["state"][0][2], np.shape(state["prev"])
        if got != want:
            raise ValueError("task state: prev must be [%d, %d] (the task's 'delta' terms x plants), not %r" % (want + (got,)))
        self._load_state("_task", self.L.npb_task_set_state, state)

    def set_features(self, columns, stack: int = 1, dtype=torch.float32, final: Optional[bool] = None, as_observation: bool = False) -> None:
        """Define what the policy reads, on the device (npb_set_features): behind every step one more launch -- two with autoreset --
        keeps a contiguous ``[n, stack, len(columns)]`` tensor of every plant's last ``stack`` frames, ``[:, -1]`` the newest.  Nothing is
        read back.
        ``columns``: 1 to 64, each a column word or ``(word, options)``.  Words are keyed as ``set_task`` keys its columns: a state member,
        ``("info", name)``, ``("obs", i)``, ``"reward"``, ``"flags"``, ``"done"``, ``"maintenance"``, ``("work_order" | "completed",
        key_index)`` and, while a task is set, ``"task_reward"``.  ``options``: ``{"scale": s, "ref": r}`` gives ``(v - r) * s`` with r a
        number or a second column word (a setpoint error); ``{"bits": mask}`` on an integer column gives 1.0 where any of the bits is set;
        then ``"nan_to"`` replaces a NaN and ``"clip": (lo, hi)`` clips; ``"fresh"`` (default 0.0) is the raw value a side column takes in
        the frame of a plant that has just been restarted -- its reward, info and flags still describe the terminal transition; state
        members and the observation are read live there.  ``dtype``: ``torch.float32`` or ``torch.float64``; ``stack * len(columns) <=
        256``.  ``nuclear_sim_amd.features`` is the same in numpy, bit for bit, and ``features.spec_from_stats`` turns a dry run's column
        statistics into ``ref`` / ``scale``.
        A plant's stack restarts with its episode: the same-step autoreset refills it with the frame of the restored state, and the stack
        that ended -- the terminal frame included -- is kept in ``final_features()`` (``final``: default on with autoreset); ``reset``,
        ``restore`` and ``restore_from_bank`` refill the plants they reset.  With features on ``step()`` adds ``info["features"]`` and,
        with autoreset, ``info["final_features"]``; with ``as_observation`` it returns the features in place of the observation (which
        stays in ``info["observation"]``).  ``set_features(None)`` turns it off."""
        self._refuse_under_rollout("the features")
        if columns is None:
            if self._feat is not None:
                _lib.check(self.L.npb_set_features(self._h, None), self._h)
            self._feat = None
            return
        ms = self._msum
        req = _lib.features_request(columns, stack, dtype, INFO_COLUMNS, self._task is not None, 0 if ms is None else len(ms["keys"]), self._n_controls(), self._n_orders())      # a bad word is refused here
        if not hasattr(self.L, "npb_set_features"):
            raise _lib.NpbError("libnpb.so has no npb_set_features: rebuild")
        spec, rows, buffers = req["spec"], req["columns"], self._side_buffers()
        C = len(spec["columns"])
        cols = (_lib.NpbFeatureColumn * C)()
        for k, D in enumerate(spec["columns"]):
            F = cols[k]
            self._fill_column(F.column, buffers, rows[D["col"]])
            F.kind, F.mask, F.scale, F.lo, F.hi, F.nan_to, F.fresh = _lib.FEATURE_KINDS[D["kind"]], D["mask"], D["scale"], D["lo"], D["hi"], D["nan_to"], D["fresh"]
            F.fresh_live = int(D["live"])
            if isinstance(D["ref"], tuple):
                F.ref_from_column, F.ref, F.ref_fresh_live = 1, D["ref_fresh"], int(D["ref_live"])
                self._fill_column(F.ref_column, buffers, rows[D["ref"][1]])
            else:
                F.ref = D["ref"]
        tdtype = torch.float64 if spec["dtype"] == "float64" else torch.float32
        keep_final = (self._episode is not None) if final is None else bool(final)
        with torch.cuda.device(self.device):
            out = torch.zeros((self.n, spec["stack"], C), dtype=tdtype, device=self.device)
            fin = torch.zeros((self.n, spec["stack"], C), dtype=tdtype, device=self.device) if keep_final else None
        d = _lib.NpbFeaturesDesc()
        d.n_columns, d.columns, d.stack, d.out_type = C, cols, spec["stack"], _lib.FEATURE_DTYPES[spec["dtype"]]
        d.out, d.final = out.data_ptr(), None if fin is None else fin.data_ptr()
        _lib.check(self.L.npb_set_features(self._h, ctypes.byref(d)), self._h)      # (refused: what was set before stays)
        self._feat = dict(self._reading(req, buffers), out=out, final=fin, request=req, as_observation=bool(as_observation), unprimed=True,
                          state=(("primed", np.int32, (self.n,)), ("seen", np.int32, (self.n,))))

    def features(self) -> torch.Tensor:
        """The ``[n, stack, n_columns]`` tensor, the same storage on every call and current after every ``step``.  Plants without a frame
        yet -- before the first step, after ``clear_features`` -- first get the frame of their current state in every slot
        (npb_features_prime)."""
        ft = self._on("_feat")
        if ft["unprimed"]:
            self.get_observation()      # (a fresh frame reads the observation live)
            _lib.check(self.L.npb_features_prime(self._h, self._stream()), self._h)
            ft["unprimed"] = False
        return ft["out"]

    def final_features(self) -> torch.Tensor:
        """``[n, stack, n_columns]``: row p is the stack, terminal frame included, of the last episode of plant p that the autoreset ended;
        the rows of the other plants stay as they were (as ``info["final_observation"]``)"""
        ft = self._on("_feat")
        if ft["final"] is None:
            raise _lib.NpbError("no final features: set_features(..., final=True), with autoreset")
        return ft["final"]

    def clear_features(self, mask=None) -> None:
        """the masked plants (None = all) unprimed: their next frame fills every slot of their stack (npb_features_clear)"""
        self._clear("_feat", self.L.npb_features_clear, mask)["unprimed"] = True

    def _after_restart(self, mask) -> None:
        """behind ``reset`` / ``restore`` / ``restore_from_bank``, THE place where an attachment follows a restart the caller made: the
        plants they reset show the features' frame of their new state, start a new hold of the controls -- and with it their order rules
        anew, which follow the hold's restart words and keep none of their own -- and have their episode cut in the rollout's last
        recorded slot"""
        if self._feat is not None:
            self.clear_features(mask)
            self.features()
        if self._ctl is not None:
            self.clear_controls(mask)
        if self._roll is not None:
            _lib.check(self.L.npb_rollout_cut(self._h, self._p(mask), self._stream()), self._h)
        # the normaliser needs nothing new here: a restart bumps the carried episode index, and a changed index restarts the return's
        # carry.  Only a handle without autoreset carries no index: there the plants are unprimed, as the features' are above
        if self._norm is not None and self._norm["reward"] is not None and self._episode is None:
            self.clear_normalizer(mask)

    def features_state(self) -> Dict[str, np.ndarray]:
        """The features' own state for a checkpoint (npb_features_get_state), beside ``state_arrays()`` and a copy of ``features()``:
        ``primed`` and ``seen`` int32 [n] (the plant has a frame; the episode index last seen)."""
        return self._get_state("_feat", self.L.npb_features_get_state)

    def load_features_state(self, state, stack=None) -> None:
        """put back what ``features_state()`` returned (npb_features_set_state) and, with ``stack``, a saved copy of ``features()``"""
        ft = self._on("_feat")
        primed = self._load_state("_feat", self.L.npb_features_set_state, state)[0]
        if stack is not None:
            ft["out"].copy_(torch.as_tensor(stack).to(device=self.device, dtype=ft["out"].dtype).reshape(ft["out"].shape))
        ft["unprimed"] = not bool(primed.all())

    def features_spec(self) -> dict:
        """the request as data: {"columns": what each row read is (``_lib.column_word``), "spec": what ``nuclear_sim_amd.features`` takes
        over those rows}"""
        return self._on("_feat")["request"]

    def features_samples(self) -> torch.Tensor:
        """The rows the features read as they are NOW, widened to float64, [n_rows, n] on the device (gather launches and copies: for checks
        and debugging, not for the hot path), as ``task_samples`` gives the task's."""
        return self._column_samples(self._on("_feat")["request"]["columns"])

    def set_normalizer(self, columns="all", reward=None, eps: float = 1e-8) -> None:
        """Running observation and reward normalisation on the device (npb_set_normalizer), what ``VecNormalize`` gives a PPO loop: while
        it is on and training every ``step()`` folds this step's raw samples of the chosen feature columns into running statistics
        (count, mean, M2) -- two launches more, nothing read back, the order of every addition pinned -- and rewrites ``ref = mean`` and
        ``scale = 1 / sqrt(var + eps)`` of those columns in front of the features' frame of that step; the options a column was given in
        ``set_features`` are where it starts from, and its ``"clip"`` is the clip of the normalised value.
        ``columns``: ``"all"`` (every eligible column: affine with a constant ref), a list of indices into the features' columns, or None.
        ``reward``: None, or ``{"gamma": g, "clip": c}``: a per-plant discounted return is kept (it restarts with the episode), its
        running spread scales the reward -- no mean is subtracted -- and ``step()`` adds ``info["norm_reward"]``; a rollout
        (``set_rollout``, set AFTER the normaliser) records that in place of the reward, while ``info["episode_return"]`` and the episode
        records keep the raw one.  The reward is the task's while a task is set.  ``columns=None`` with ``reward=None`` turns it off, and
        the features get their own ``ref`` / ``scale`` back.  ``nuclear_sim_amd.normalizer`` is the same in numpy, bit for bit."""
        if self._roll is not None:
            raise _lib.NpbError("the rollout records the reward the normaliser would change: set_rollout(None) first, then the normaliser, then the rollout")
        if columns is None and reward is None:
            if self._norm is not None:
                _lib.check(self.L.npb_set_normalizer(self._h, None), self._h)
            self._norm = None
            return
        ft = self._feat
        spec = None if ft is None else ft["request"]["spec"]
        if isinstance(columns, str):
            if columns != "all":
                raise ValueError("columns is 'all', a list of feature column indices or None, not %r" % (columns,))
            columns = [] if spec is None else [j for j, D in enumerate(spec["columns"]) if D["kind"] == "affine" and not isinstance(D["ref"], tuple)]
        columns = [] if columns is None else [int(j) for j in columns]
        normalizer.check(spec, columns, reward, eps)      # a bad request is refused here
        if not hasattr(self.L, "npb_set_normalizer"):
            raise _lib.NpbError("libnpb.so has no npb_set_normalizer: rebuild")
        d = _lib.NpbNormalizerDesc()
        idx = (ctypes.c_int * max(len(columns), 1))(*columns)
        d.n_columns, d.columns, d.eps = len(columns), idx, float(eps)
        out = None
        if reward is not None:
            with torch.cuda.device(self.device):
                out = torch.zeros(self.n, dtype=torch.float64, device=self.device)
            d.reward, d.gamma, d.clip, d.norm_reward = 1, float(reward["gamma"]), float(reward["clip"]), out.data_ptr()
        _lib.check(self.L.npb_set_normalizer(self._h, ctypes.byref(d)), self._h)      # (refused: what was set before stays)
        S, n = len(columns) + (reward is not None), self.n if reward is not None else 0
        reads = frozenset(["task_reward"] if reward is not None and self._task is not None else [])
        self._norm = {"norm_reward": out, "columns": columns, "reward": None if reward is None else dict(reward), "eps": float(eps),
                      "reads": reads, "holds": [self._task["reward"]] if reads else [],
                      "state": (("count", np.float64, (S,)), ("mean", np.float64, (S,)), ("M2", np.float64, (S,)), ("ret", np.float64, (n,)),
                                ("primed", np.int32, (n,)), ("seen", np.int32, (n,)), ("ended", np.int32, (n,)))}

    def normalizer_training(self, on: bool = True) -> None:
        """``False`` freezes the statistics for evaluation (npb_normalizer_training): no fold, the features keep the table as it stands;
        the reward is still normalised, with the frozen scale, and the return is still carried"""
        self._on("_norm")
        _lib.check(self.L.npb_normalizer_training(self._h, int(bool(on))), self._h)

    def normalizer_state(self) -> Dict[str, np.ndarray]:
        """The normaliser's own state for a checkpoint (npb_normalizer_get_state): ``count``, ``mean``, ``M2`` float64 [S], and with the
        return stream ``ret`` float64 [n], ``primed``, ``seen``, ``ended`` int32 [n] (else empty)."""
        return self._get_state("_norm", self.L.npb_normalizer_get_state)

    def load_normalizer_state(self, state) -> None:
        """put back what ``normalizer_state()`` returned (npb_normalizer_set_state); the features' table follows.  A dry run's statistics
        warm-start a run this way."""
        self._load_state("_norm", self.L.npb_normalizer_set_state, state)

    # ---- one normaliser across shards (npb_normalizer_shard_delta, npb_normalizer_apply_shards; normalizer.shard_delta / combine)
    def _norm_streams(self) -> int:
        """S of the set normaliser, for the calls that synchronise shards"""
        nm = self._on("_norm")
        if not hasattr(self.L, "npb_normalizer_apply_shards"):
            raise _lib.NpbError("libnpb.so has no npb_normalizer_apply_shards: rebuild")
        return len(nm["columns"]) + (nm["reward"] is not None)

    def normalizer_shard_delta(self) -> torch.Tensor:
        """What this shard folded since the last synchronisation, a device float64 [3, S] -- count, mean, M2 -- with nothing read back
        (npb_normalizer_shard_delta): zeros for a shard that is frozen or did not step.  ``normalizer.shard_delta`` is the same in numpy,
        bit for bit."""
        S = self._norm_streams()
        with torch.cuda.device(self.device):
            out = torch.zeros((3, S), dtype=torch.float64, device=self.device)
        _lib.check(self.L.npb_normalizer_shard_delta(self._h, ctypes.c_void_p(out.data_ptr()), self._stream()), self._h)
        return out

    def normalizer_apply_shards(self, deltas) -> None:
        """The base merged with W shards' deltas, a contiguous device float64 [W, 3, S] in shard order (npb_normalizer_apply_shards): the
        result is this handle's state and its new base, and the features' table and the reward's scale follow it.  Every shard that
        applies the same deltas holds the same bits.  Allowed while frozen.  ``normalizer.combine`` is the same in numpy."""
        S = self._norm_streams()
        if not isinstance(deltas, torch.Tensor) or deltas.dtype != torch.float64 or deltas.dim() != 3 or tuple(deltas.shape[1:]) != (3, S) or \
                not 1 <= deltas.shape[0] <= _lib.PPO_SHARDS_MAX or not deltas.is_contiguous() or deltas.device != self.device:
            raise ValueError("deltas must be a contiguous float64 [W, 3, %d] tensor on %s, W 1 .. %d" % (S, self.device, _lib.PPO_SHARDS_MAX))
        _lib.check(self.L.npb_normalizer_apply_shards(self._h, ctypes.c_void_p(deltas.data_ptr()), deltas.shape[0], self._stream()), self._h)
        self._norm["shards_held"] = deltas      # (alive while the launch reads it)

    def normalizer_sync(self, exchange) -> None:
        """One synchronisation of the running normaliser between shards, nothing read back: ``normalizer_shard_delta()``,
        ``exchange(vec)`` -- this shard's device float64 [3 S] in, the [W, 3 S] of all shards out, in shard order
        (``sharding.normalizer_exchange``) -- then ``normalizer_apply_shards``.  Afterwards every shard holds the statistics of all
        samples of all shards, bit for bit the same, and samples from before the last synchronisation are not counted again."""
        vec = self.normalizer_shard_delta()
        every = exchange(vec.reshape(-1))
        if not isinstance(every, torch.Tensor) or every.dim() != 2 or every.shape[1] != vec.numel() or not 1 <= every.shape[0] <= _lib.PPO_SHARDS_MAX:
            raise ValueError("exchange must return the [W, %d] tensor of every shard's delta, W 1 .. %d, not %r"
                             % (vec.numel(), _lib.PPO_SHARDS_MAX, tuple(every.shape) if isinstance(every, torch.Tensor) else every))
        self.normalizer_apply_shards(every.contiguous().view(every.shape[0], 3, vec.shape[1]))

    def normalizer_shard_state(self) -> Dict[str, np.ndarray]:
        """``normalizer_state()`` and ``base``, float64 [3, S]: what the shards agreed on at the last synchronisation
        (npb_normalizer_get_base).  A checkpoint of a sharded run keeps this one."""
        S = self._norm_streams()
        state = self.normalizer_state()
        base = np.zeros((3, S), dtype=np.float64)
        _lib.check(self.L.npb_normalizer_get_base(self._h, base.ctypes.data_as(ctypes.c_void_p), self._stream()), self._h)
        state["base"] = base
        return state

    def load_normalizer_shard_state(self, state) -> None:
        """put back what ``normalizer_shard_state()`` returned: the state as ``load_normalizer_state`` does, and the base"""
        S = self._norm_streams()
        base = np.ascontiguousarray(state["base"], dtype=np.float64)
        if base.shape != (3, S):
            raise ValueError("base must be [3, %d], not %r" % (S, base.shape))
        self.load_normalizer_state({k: v for k, v in state.items() if k != "base"})
        _lib.check(self.L.npb_normalizer_set_base(self._h, base.ctypes.data_as(ctypes.c_void_p), self._stream()), self._h)

    def normalizer_stats(self) -> Dict[str, np.ndarray]:
        """``count``, ``mean``, ``var`` and ``scale`` (what the features' table holds; the return stream's last) as numpy, float64 [S]"""
        z = self.normalizer_spec()
        z.load_state({k: v for k, v in self.normalizer_state().items() if v.size})
        return z.stats()

    def normalizer_spec(self) -> "normalizer.Normalizer":
        """a ``nuclear_sim_amd.normalizer.Normalizer`` as this one was set, its state at zero: the statement to compare with"""
        nm = self._on("_norm")
        return normalizer.Normalizer(None if self._feat is None else self._feat["request"]["spec"], nm["columns"], self.n, nm["reward"], nm["eps"])

    def clear_normalizer(self, mask=None) -> None:
        """the masked plants (None = all) start a new discounted return on their next step (npb_normalizer_clear).  ``reset`` / ``restore``
        need not call it: the episode index they bump does the work"""
        self._clear("_norm", self.L.npb_normalizer_clear, mask)

    def _control_readers(self):
        """what reads the controls' held / previous columns, as a refusal names them"""
        return self._readers_of(("control", "control_prev"))

    def set_controls(self, axes, interval: int = 1, dtype=torch.float32) -> None:
        """Define what the policy writes, on the device (npb_set_controls): in front of every step one more launch reads every plant's
        row of a bound ``[n, len(axes)]`` tensor, transforms each element and moves the actuators or fills the input columns the axes
        name.  Nothing is read back; nothing stands between the policy's output tensor and ``step()``.
        ``axes``: 1 to 8, each ``(target, kind)`` or ``(target, kind, options)``:
        ``("rod" | "flow" | "valve" | "boron", "rate")`` -- y is a signed magnitude, y > 0 the reference's move with the actuator's
        increasing ControlAction at magnitude y, y < 0 the decreasing one at -y; ``(actuator, "target")`` -- y is a position the actuator
        moves towards at ``max_magnitude`` per step and stops at; ``("power_setpoint" | "cooling_water_temp", "column")`` -- y is that
        plant's value of the step's input; ``(None, "value")`` -- y moves nothing and is only held, for the task and the features to read.
        ``options``: ``"scale"`` and ``"offset"`` (y = x * scale + offset), ``"clip": (lo, hi)`` (a
        rate's default is (-1, 1)), ``"nan_to"`` (default 0.0), ``"deadband"`` (rate), ``"max_magnitude"`` (target, default 1.0).
        ``interval``: K, a decoded row is held for K steps (a held target keeps moving, a held rate repeats its move); a plant's hold
        restarts with its episode, and ``reset``, ``restore`` and ``restore_from_bank`` restart it for the plants they reset.
        Several actuators may move in one step.  ``step(action, magnitude)`` still works: the step applies them behind the controls, as
        it always did.  While controls are set ``("control", a)`` and ``("control_prev", a)`` -- axis a's held and previous value -- are
        column words for ``set_task``, ``set_features``, ``enable_column_stats`` and ``enable_event_windows`` (effort: ``abs_err`` of
        ``("control", a)`` against 0; jerk: ``sq_err`` against ``("control_prev", a)``), and ``step()`` adds ``info["controls"]``, the
        held values ``[len(axes), n]``.  ``nuclear_sim_amd.controls`` is the same in numpy, bit for bit.  ``set_controls(None)`` turns
        it off."""
        self._refuse_under_rollout("the controls")
        readers = self._control_readers()      # (none without controls: their columns are no words then)
        if readers:
            raise _lib.NpbError("%s read(s) the controls' columns: turn that off first" % " and ".join(readers))
        readers = self._readers_of(("order",))      # (the controls go, set or None alike, and their order rules with them)
        if readers:
            raise _lib.NpbError("%s read(s) the order rules' columns: turn that off first" % " and ".join(readers))
        if axes is None:
            if self._ctl is not None:
                _lib.check(self.L.npb_set_controls(self._h, None), self._h)
            self._ctl = self._ord = None
            return
        spec = _lib.controls_request(axes, interval, dtype, self.params.heat_source)      # a bad axis is refused here
        if self._profile is not None and any(D["target"] == "power_setpoint" for D in spec["axes"]):
            raise ValueError("a 'power_setpoint' axis fills the column the power profile drives")
        if not hasattr(self.L, "npb_set_controls"):
            raise _lib.NpbError("libnpb.so has no npb_set_controls: rebuild")
        A = len(spec["axes"])
        cax = (_lib.NpbControlAxis * A)()
        for k, D in enumerate(spec["axes"]):
            X = cax[k]
            X.kind = _lib.CONTROL_KINDS[D["kind"]]
            X.target = 0 if D["target"] is None else (_lib.CONTROL_INPUTS if D["kind"] == "column" else _lib.CONTROL_ACTUATORS)[D["target"]]
            X.scale, X.offset, X.lo, X.hi, X.nan_to, X.deadband, X.max_magnitude = (D[name] for name in ("scale", "offset", "lo", "hi", "nan_to",
                                                                                                          "deadband", "max_magnitude"))
        tdtype = torch.float64 if spec["dtype"] == "float64" else torch.float32
        with torch.cuda.device(self.device):
            tin = torch.zeros((self.n, A), dtype=tdtype, device=self.device)
            held = torch.zeros((A, self.n), dtype=torch.float64, device=self.device)
            prev = torch.zeros((A, self.n), dtype=torch.float64, device=self.device)
        d = _lib.NpbControlsDesc()
        d.n_axes, d.axes, d.interval, d.in_type = A, cax, spec["interval"], _lib.CONTROL_DTYPES[spec["dtype"]]
        d.input, d.held, d.prev = tin.data_ptr(), held.data_ptr(), prev.data_ptr()
        _lib.check(self.L.npb_set_controls(self._h, ctypes.byref(d)), self._h)      # (refused: what was set before stays)
        self._ctl = {"in": tin, "held": held, "prev": prev, "spec": spec,
                     "state": (("held", np.float64, (A, self.n)), ("prev", np.float64, (A, self.n)), ("age", np.int32, (self.n,)),
                               ("primed", np.int32, (self.n,)), ("seen", np.int32, (self.n,)))}
        self._ord = None      # (npb_set_controls dropped the rules: they read the old axes)

    def controls_input(self) -> torch.Tensor:
        """The bound ``[n, n_axes]`` tensor the next ``step`` decodes, the same storage on every call: have the policy write into it"""
        return self._on("_ctl")["in"]

    def clear_controls(self, mask=None) -> None:
        """the masked plants (None = all) unprimed: their next step starts a new hold (npb_controls_clear)"""
        self._clear("_ctl", self.L.npb_controls_clear, mask)

    def controls_state(self) -> Dict[str, np.ndarray]:
        """The controls' own state for a checkpoint (npb_controls_get_state), beside ``state_arrays()``: ``held`` and ``prev`` float64
        [n_axes, n], ``age``, ``primed`` and ``seen`` int32 [n]."""
        return self._get_state("_ctl", self.L.npb_controls_get_state)

    def load_controls_state(self, state) -> None:
        """put back what ``controls_state()`` returned (npb_controls_set_state)"""
        self._load_state("_ctl", self.L.npb_controls_set_state, state)

    def controls_spec(self) -> dict:
        """the request as data: what ``nuclear_sim_amd.controls.Decoder`` takes"""
        return self._on("_ctl")["spec"]

    def set_control_orders(self, orders) -> None:
        """Let the policy order maintenance (npb_set_control_orders): rules on the controls' ``"value"`` axes.  Behind the decode of every
        step, and in front of the step, one more launch looks at the held value y of each rule's axis: where the plant's row was read on
        this step, ``y > threshold`` and the rule has not fired on the plant for ``min_interval`` steps (or not since its restart), the
        plant gets the rule's service -- by bits what ``perform_maintenance`` / ``perform_component_maintenance`` /
        ``perform_turbine_maintenance`` would do to it, with the same record in the maintenance log.  Nothing is read back.
        ``orders``: 1 to 8, each ``(axis, component, action)`` or ``(axis, component, action, options)``.  ``axis``: the index of a
        ``(None, "value")`` axis of ``set_controls``; several rules may share one and are applied in their order.  ``component``:
        ``"pump"``, ``"steam_generator"``, ``"steam_generator_system"``, ``"condenser"``, ``"ejector"``, ``"turbine"``, ``"bearing"``,
        ``"lubrication"`` or ``"stage"``.  ``action``: a name of ``_lib.MAINT_ACTIONS``, ``_lib.COMPONENT_ACTIONS`` or
        ``_lib.TURBINE_ACTIONS`` for that component, or its catalog index; a handler that is not offered is refused as the ``perform_*``
        methods refuse it.  ``options``: ``"unit"`` (the pump 0..3, generator, ejector, bearing or stage; default 0), ``"threshold"``
        (default 0.0), ``"min_interval"`` (default 1), ``"bearing"`` (a pump's bearing replacement), ``"target_level"`` (a pump's oil
        top-off, default 95.0), ``"cleaning_type"`` (steam generators, condenser, ejectors).  A rule that cannot succeed on this env --
        a unit that does not exist, an action without a handler, a component the mode does not step, an axis that is no ``"value"``
        axis -- is refused here, so a firing is a success.
        A held row (``interval`` > 1) orders once, on the step it was read.  A plant's rules restart with its hold: a new episode,
        ``reset``, ``restore``, ``restore_from_bank`` and ``clear_controls`` let every rule fire again at once.
        While rules are set ``("order", r)`` -- 1.0 where rule r fired on this step, else 0.0 -- is a column word for ``set_task`` (the
        price of an order), ``set_features`` (an input of the policy), ``enable_column_stats`` and ``enable_event_windows`` (a window
        around an order), and ``step()`` adds ``info["orders"]``, ``[len(orders), n]``.  ``nuclear_sim_amd.controls.Orders`` is the same
        in numpy, bit for bit.  ``set_control_orders(None)`` turns it off; ``set_controls`` drops the rules."""
        if self._pol is not None:
            raise _lib.NpbError("the policy reads or writes the controls every step: set_policy(None) first")
        readers = self._readers_of(("order",))      # (none without rules: their column is no word then)
        if readers:
            raise _lib.NpbError("%s read(s) the order rules' columns: turn that off first" % " and ".join(readers))
        if orders is None:
            if self._ord is not None:
                _lib.check(self.L.npb_set_control_orders(self._h, None), self._h)
            self._ord = None
            return
        rules = _lib.control_orders_request(orders)      # a bad word is refused here
        ctl = self._on("_ctl")
        mode = controls.MODES[self.params.mode]
        controls.orders_check(rules, ctl["spec"], self.n, mode)      # and what this env cannot carry out here
        if not hasattr(self.L, "npb_set_control_orders"):
            raise _lib.NpbError("libnpb.so has no npb_set_control_orders: rebuild")
        R = len(rules)
        table = (_lib.NpbControlOrder * R)()
        for k, D in enumerate(rules):
            X = table[k]
            X.axis, X.family, X.action, X.unit, X.option = D["axis"], _lib.ORDER_FAMILIES[D["family"]], D["action"], D["unit"], D["option"]
            X.min_interval, X.amount, X.threshold = int(D["min_interval"]), D["amount"], D["threshold"]
        with torch.cuda.device(self.device):
            fired = torch.zeros((R, self.n), dtype=torch.float64, device=self.device)
        d = _lib.NpbControlOrdersDesc()
        d.n_orders, d.orders, d.fired = R, table, fired.data_ptr()
        _lib.check(self.L.npb_set_control_orders(self._h, ctypes.byref(d)), self._h)      # (refused: what was set before stays)
        self._ord = {"fired": fired, "rules": rules, "mode": mode, "state": (("since", np.int32, (R, self.n)),)}

    def control_orders(self) -> Dict[str, object]:
        """``{"fired": the device float64 [R, n] of the last step (1.0 where rule r fired), "since": int32 [R, n] as numpy -- the steps
        since rule r last fired on the plant, 1 on the step it fired, ``controls.NEVER`` where it has not since the plant's restart}``"""
        return {"fired": self._on("_ord")["fired"], "since": self.control_orders_state()["since"]}

    def control_orders_state(self) -> Dict[str, np.ndarray]:
        """The order rules' own state for a checkpoint (npb_control_orders_get_state), beside ``controls_state()``: ``since`` int32 [R, n]"""
        return self._get_state("_ord", self.L.npb_control_orders_get_state)

    def load_control_orders_state(self, state) -> None:
        """put back what ``control_orders_state()`` returned (npb_control_orders_set_state)"""
        self._load_state("_ord", self.L.npb_control_orders_set_state, state)

    def control_orders_spec(self) -> "controls.Orders":
        """a ``nuclear_sim_amd.controls.Orders`` as these rules were set, every ``since`` at NEVER: the statement to compare with"""
        od = self._on("_ord")
        return controls.Orders(od["rules"], self._on("_ctl")["spec"], self.n, od["mode"])

    def _refuse_under_rollout(self, what: str) -> None:
        """``set_features`` / ``set_controls`` while a rollout is set, set and None alike: its pre kernel copies their tensors every step,
        in the shapes it was bound with"""
        if self._pol is not None:
            raise _lib.NpbError("the policy reads or writes %s every step: set_policy(None) first" % what)
        if self._roll is not None:
            raise _lib.NpbError("the rollout records %s every step: set_rollout(None) first" % what)

    def set_rollout(self, horizon, extras: int = 0, final_rows: Optional[int] = None) -> None:
        """Record trajectories on the device (npb_set_rollout): for ``horizon`` steps (1 to 4096) every ``step()`` writes slot t of
        time-major tensors the env keeps -- two launches more, nothing read back: ``obs`` [T, n, K, C], the features as the policy saw them
        in front of the step (so features must be set; plants without a frame are primed first); ``act`` [T, n, A], the controls input as
        it wrote it (with controls set); ``extra`` [T, n, extras] float32, a copy of ``rollout_extras_input()``, [n, extras], which the
        caller writes before each step (value, log-probability, ...; up to 8); ``reward`` [T, n] float64 (the task's while a task is set);
        ``ended`` [T, n] uint8 (bit 0 terminated, bit 1 truncated, bit 2 cut: ``reset`` / ``restore`` / ``restore_from_bank`` between two
        steps cut the plants they reset); ``episode`` [T, n] int32 (-1 without autoreset); and for every truncated transition
        ``final_obs[final_row[t, p]]``, its terminal stack, whose value a learner bootstraps from (``final_rows`` per plant: default the
        derived bound ceil(horizon / max_episode_steps), or 0 where nothing truncates).  A step at t == horizon is refused:
        ``rollout_begin()`` rewinds.  ``rollout_advantages`` forms GAE advantages and returns over the recorded slots in one launch.
        While the rollout is set ``set_features`` and ``set_controls`` are refused.  ``nuclear_sim_amd.rollout`` is the same in numpy, bit
        for bit.  ``set_rollout(None)`` turns it off."""
        if self._pol is not None:
            raise _lib.NpbError("the policy writes the rollout's extras every step: set_policy(None) first")
        if horizon is None:
            if self._roll is not None:
                _lib.check(self.L.npb_set_rollout(self._h, None), self._h)
            self._roll = None
            return
        ft, ct = self._feat, self._ctl
        if ft is None:
            raise _lib.NpbError("a rollout records the features: set_features() first")
        if not hasattr(self.L, "npb_set_rollout"):
            raise _lib.NpbError("libnpb.so has no npb_set_rollout: rebuild")
        T, E = int(horizon), int(extras)
        if not 1 <= T <= _lib.ROLLOUT_HORIZON_MAX:
            raise ValueError("a rollout's horizon is 1 to %d steps, not %r" % (_lib.ROLLOUT_HORIZON_MAX, horizon))
        if not 0 <= E <= _lib.ROLLOUT_EXTRAS_MAX:
            raise ValueError("a rollout takes 0 to %d extras, not %r" % (_lib.ROLLOUT_EXTRAS_MAX, extras))
        R = rollout.final_rows_bound(T, self._max_episode_steps) if final_rows is None else int(final_rows)
        if R < 0:
            raise ValueError("final_rows must be >= 0")
        n, (_, K, C) = self.n, ft["out"].shape
        A = 0 if ct is None else ct["in"].shape[1]
        with torch.cuda.device(self.device):
            def zeros(shape, dtype):
                return torch.zeros(shape, dtype=dtype, device=self.device)
            t = {"obs": zeros((T, n, K, C), ft["out"].dtype), "act": zeros((T, n, A), ct["in"].dtype) if A else None,
                 "extra": zeros((T, n, E), torch.float32) if E else None, "reward": zeros((T, n), torch.float64),
                 "ended": zeros((T, n), torch.uint8), "episode": zeros((T, n), torch.int32), "final_row": zeros((T, n), torch.int32),
                 "final_obs": zeros((n * R, K, C), ft["out"].dtype) if R else None}
            extras_in = zeros((n, E), torch.float32) if E else None
        d = _lib.NpbRolloutDesc()
        d.horizon, d.n_extras, d.final_rows, d.extras_in = T, E, R, None if extras_in is None else extras_in.data_ptr()
        for name, x in t.items():
            setattr(d, name, None if x is None else x.data_ptr())
        _lib.check(self.L.npb_set_rollout(self._h, ctypes.byref(d)), self._h)      # (refused: what was set before stays)
        self._roll = {"tensors": t, "extras_in": extras_in, "out": {},
                      "spec": {"horizon": T, "extras": E, "final_rows": R, "stack": (K, C), "axes": A, "autoreset": self._episode is not None,
                               "max_episode_steps": self._max_episode_steps, "obs_dtype": str(ft["out"].dtype).split(".")[1],
                               "act_dtype": None if ct is None else str(ct["in"].dtype).split(".")[1]}}

    def rollout_extras_input(self) -> torch.Tensor:
        """The bound ``[n, extras]`` float32 tensor whose rows the next ``step`` copies into ``extra[t]``, the same storage on every call"""
        x = self._on("_roll")["extras_in"]
        if x is None:
            raise _lib.NpbError("no extras: set_rollout(..., extras=E)")
        return x

    def rollout(self) -> dict:
        """The recorded tensors, the same storage on every call (``act``, ``extra`` and ``final_obs`` None where there are none), and
        ``"t"``, the number of slots recorded"""
        return dict(self._on("_roll")["tensors"], t=int(self.L.npb_rollout_steps(self._h)))

    def rollout_begin(self) -> None:
        """rewind: t = 0, every row of ``final_obs`` free again, ``final_row`` -1 (npb_rollout_begin)"""
        self._on("_roll")
        _lib.check(self.L.npb_rollout_begin(self._h, self._stream()), self._h)

    def rollout_advantages(self, gamma: float, lam: float, values=None, last_value=None, final_values=None, dtype=torch.float32):
        """GAE advantages and returns over the recorded slots in one launch (npb_rollout_advantages): ``(adv, ret)``, each ``[t, n]`` of
        ``dtype`` (float32 or float64), views of tensors the env keeps per dtype.  ``values``: None (0 everywhere: with ``lam`` 1 ``ret`` is the
        discounted return-to-go), a float32 ``[>= t, n]`` tensor, or ``("extra", j)`` -- column j of the recorded extras, read in place.
        ``last_value``: float32 [n], the value of the state behind the last slot; ``final_values``: float32 [n * final_rows], the caller's
        value of every row of ``final_obs`` (needed when final_rows > 0): a truncated transition bootstraps from the value of its TERMINAL
        state, a terminated or cut one from 0.  Double arithmetic, as ``nuclear_sim_amd.rollout.advantages`` states it, bit for bit."""
        ro = self._on("_roll")
        T, tensors = ro["spec"]["horizon"], ro["tensors"]
        name = {torch.float32: "float32", torch.float64: "float64"}.get(dtype)
        if name is None:
            raise ValueError("advantages are float32 or float64, not %r" % (dtype,))

        def column(x, what, shape=None):      # a float32 device tensor of the caller's, as it is when it can be
            if x is None:
                return None
            x = torch.as_tensor(x).to(device=self.device, dtype=torch.float32).contiguous()
            if shape is not None and tuple(x.shape) != shape:
                raise ValueError("%s must be %r, not %r" % (what, shape, tuple(x.shape)))
            return x
        d = _lib.NpbRolloutAdvantagesDesc()
        d.gamma, d.lam, d.out_type = float(gamma), float(lam), _lib.ROLLOUT_DTYPES[name]
        if isinstance(values, tuple):
            if len(values) != 2 or values[0] != "extra" or tensors["extra"] is None or not 0 <= int(values[1]) < ro["spec"]["extras"]:
                raise ValueError("values in place: ('extra', j) with j one of the rollout's %d extras, not %r" % (ro["spec"]["extras"], values))
            E = ro["spec"]["extras"]
            d.value, d.value_time_stride, d.value_plant_stride = tensors["extra"].data_ptr() + 4 * int(values[1]), self.n * E, E
            values = None
        else:
            values = column(values, "values")
            if values is not None:
                if values.dim() != 2 or values.shape[1] != self.n or values.shape[0] < int(self.L.npb_rollout_steps(self._h)):
                    raise ValueError("values must be [>= t, n], not %r" % (tuple(values.shape),))
                d.value, d.value_time_stride, d.value_plant_stride = values.data_ptr(), self.n, 1
        last_value = column(last_value, "last_value", (self.n,))
        final_values = column(final_values, "final_values", (self.n * ro["spec"]["final_rows"],))
        d.last_value = None if last_value is None else last_value.data_ptr()
        d.final_value = None if final_values is None else final_values.data_ptr()
        if name not in ro["out"]:
            with torch.cuda.device(self.device):
                ro["out"][name] = (torch.zeros((T, self.n), dtype=dtype, device=self.device), torch.zeros((T, self.n), dtype=dtype, device=self.device))
        adv, ret = ro["out"][name]
        d.adv, d.ret = adv.data_ptr(), ret.data_ptr()
        _lib.check(self.L.npb_rollout_advantages(self._h, ctypes.byref(d), self._stream()), self._h)
        ro["held"] = (values, last_value, final_values)      # (alive while the launch reads them)
        t = int(self.L.npb_rollout_steps(self._h))
        ro["last"] = (adv[:t], ret[:t])      # (what ``rollout_moments`` and ``rollout_minibatches`` take by default)
        return adv[:t], ret[:t]

    def rollout_spec(self) -> dict:
        """the request as data: what ``nuclear_sim_amd.rollout.Recorder`` takes"""
        return self._on("_roll")["spec"]

    _MB_DTYPES = {torch.float32: "float32", torch.float64: "float64"}

    def _last_advantages(self, ro, advantages=None):
        """``(adv, ret)`` a minibatch or the moments are taken of: the caller's pair, else what the last ``rollout_advantages`` formed"""
        if advantages is None:
            advantages = ro.get("last")
            if advantages is None:
                raise _lib.NpbError("no advantages formed yet: rollout_advantages() first, or pass advantages=(adv, ret)")
        adv, ret = advantages
        t = int(self.L.npb_rollout_steps(self._h))
        for name, x in (("adv", adv), ("ret", ret)):
            if not isinstance(x, torch.Tensor) or x.device != self.device or x.dtype != adv.dtype or x.dtype not in self._MB_DTYPES:
                raise ValueError("%s must be a float32 or float64 tensor on %s, of adv's type" % (name, self.device))
            if x.dim() != 2 or x.shape[1] != self.n or x.shape[0] < t or not x.is_contiguous():
                raise ValueError("%s must be a contiguous [>= t, n] = [>= %d, %d] tensor, not %r" % (name, t, self.n, tuple(x.shape)))
        return adv, ret, t

    def rollout_moments(self, x=None, ddof: int = 1) -> torch.Tensor:
        """``(count, mean, var, std)`` of ``x``, a contiguous [rows, cols] float32 or float64 device tensor (default: the advantages the
        last ``rollout_advantages`` formed), as a device float64 [4] tensor: nothing is read back (npb_rollout_moments).  The order of
        every addition is pinned -- rows in order down each column, then a tree of groups of 256 over the columns -- so the bits are
        ``nuclear_sim_amd.rollout.moments``'s, whatever the launch geometry.  Any tensor will do: no rollout need be set for one given."""
        if not hasattr(self.L, "npb_rollout_moments"):
            raise _lib.NpbError("libnpb.so has no npb_rollout_moments: rebuild")
        if x is None:
            adv, _, t = self._last_advantages(self._on("_roll"))
            x = adv[:t]
        if not isinstance(x, torch.Tensor) or x.device != self.device or x.dim() != 2 or x.dtype not in self._MB_DTYPES or not x.is_contiguous():
            raise ValueError("moments are taken of a contiguous [rows, cols] float32 or float64 tensor on %s" % (self.device,))
        rows, cols = x.shape
        if int(ddof) < 0 or rows * cols <= int(ddof):
            raise ValueError("rows * cols = %d must exceed ddof = %d" % (rows * cols, int(ddof)))
        with torch.cuda.device(self.device):
            out = torch.zeros(4, dtype=torch.float64, device=self.device)
        d = _lib.NpbMomentsDesc()
        d.src, d.type, d.ddof, d.rows, d.cols, d.out = x.data_ptr(), _lib.ROLLOUT_DTYPES[self._MB_DTYPES[x.dtype]], int(ddof), rows, cols, out.data_ptr()
        _lib.check(self.L.npb_rollout_moments(self._h, ctypes.byref(d), self._stream()), self._h)
        self._moments_held = x      # (alive while the launches read it)
        return out

    def rollout_moments_shards(self, exchange, x=None, ddof: int = 1) -> torch.Tensor:
        """``(count, mean, var, std)`` over ALL shards' ``x`` (default: the advantages the last ``rollout_advantages`` formed) as a device
        float64 [4] tensor, the same bits on every shard, nothing read back: this shard's part (npb_rollout_moments_part), the combine
        (npb_rollout_moments_combine), the part around the global mean, the combine.  ``exchange(vec)`` takes this shard's device
        float64 [2] and returns the [W, 2] of all shards in shard order (``sharding.ppo_exchange`` serves); it is called twice.  With one
        shard the result is ``rollout_moments``'s, bit for bit.  ``nuclear_sim_amd.rollout.moments_shards`` is the same in numpy.  A
        total count that does not exceed ``ddof`` cannot be seen without a read-back: the variance is then an infinity or a NaN."""
        if not hasattr(self.L, "npb_rollout_moments_part"):
            raise _lib.NpbError("libnpb.so has no npb_rollout_moments_part: rebuild")
        if x is None:
            adv, _, t = self._last_advantages(self._on("_roll"))
            x = adv[:t]
        if not isinstance(x, torch.Tensor) or x.device != self.device or x.dim() != 2 or x.dtype not in self._MB_DTYPES or not x.is_contiguous():
            raise ValueError("moments are taken of a contiguous [rows, cols] float32 or float64 tensor on %s" % (self.device,))
        rows, cols = x.shape
        if rows * cols < 1:
            raise ValueError("rows * cols must be >= 1")
        if int(ddof) < 0:
            raise ValueError("ddof must be >= 0")
        with torch.cuda.device(self.device):
            out = torch.zeros(4, dtype=torch.float64, device=self.device)
            parts = [torch.zeros(2, dtype=torch.float64, device=self.device) for _ in range(2)]
        d = _lib.NpbMomentsDesc()
        d.src, d.type, d.ddof, d.rows, d.cols, d.out = x.data_ptr(), _lib.ROLLOUT_DTYPES[self._MB_DTYPES[x.dtype]], 0, rows, cols, out.data_ptr()
        held = [x, out] + parts
        for squares, part in enumerate(parts):
            _lib.check(self.L.npb_rollout_moments_part(self._h, ctypes.byref(d), squares, ctypes.c_void_p(part.data_ptr()), self._stream()), self._h)
            every = exchange(part)
            if not isinstance(every, torch.Tensor) or every.dim() != 2 or every.shape[1] != 2 or not 1 <= every.shape[0] <= _lib.PPO_SHARDS_MAX or \
                    every.dtype != torch.float64 or every.device != self.device:
                raise ValueError("exchange must return the float64 [W, 2] tensor of every shard's part on %s, W 1 .. %d"
                                 % (self.device, _lib.PPO_SHARDS_MAX))
            every = every.contiguous()
            held.append(every)
            _lib.check(self.L.npb_rollout_moments_combine(self._h, ctypes.c_void_p(every.data_ptr()), every.shape[0], squares, int(ddof),
                                                          ctypes.c_void_p(out.data_ptr()), self._stream()), self._h)
        self._moments_held = held      # (alive while the launches read them)
        return out

    def rollout_permutation(self, N: int, keys, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """entries ``first .. first + count`` of the permutation of range(N) under ``keys`` (``rollout.permutation_keys(seed, epoch)``)
        as a device int32 tensor (npb_rollout_permutation): ``nuclear_sim_amd.rollout.permutation``, entry by entry"""
        count = int(N) - int(first) if count is None else int(count)
        k = (ctypes.c_uint32 * _lib.MINIBATCH_ROUNDS)(*[int(v) for v in keys])
        with torch.cuda.device(self.device):
            out = torch.zeros(max(count, 1), dtype=torch.int32, device=self.device)
        _lib.check(self.L.npb_rollout_permutation(self._h, int(N), k, int(first), count, out.data_ptr(), self._stream()), self._h)
        return out[:count]

    def rollout_minibatches(self, batch_size, epochs: int = 1, seed: int = 0, first_epoch: int = 0, normalize: bool = True, eps: float = 1e-8,
                            ddof: int = 1, unit: str = "transition", drop_last: bool = False, advantages=None, max_blocks: int = 0, moments=None):
        """Shuffled minibatches of the recorded slots, gathered on the device (npb_rollout_minibatch): a generator of dicts ``{"index",
        "obs", "act", "extra", "adv", "ret", "epoch"}``, one launch each on the env's stream and no host synchronisation.
        ``unit="transition"``: every epoch is a permutation of the t * n recorded cells; ``index`` [count] is the flat cell s * n + p and
        ``obs`` [count, K, C], ``act`` [count, A], ``extra`` [count, E], ``adv``, ``ret`` [count] its rows.  ``unit="plant"`` (recurrent
        policies): a permutation of the plants, every tensor time-major with the sequences whole, [t, count, ...].  The order of epoch e is
        a function of ``(seed, e)`` alone (``rollout.permutation_keys``; epochs ``first_epoch .. first_epoch + epochs``), so an epoch is
        resumed from three numbers.  ``normalize``: the advantages' moments are formed once (``rollout_moments``, ``ddof``) and ``adv`` is
        ``((double)adv - mean) / (std + eps)``, narrowed once.  ``advantages``: ``(adv, ret)`` [>= t, n] device tensors of one type,
        default what the last ``rollout_advantages`` returned.  A short last batch is yielded unless ``drop_last``.  ``moments``: a
        device float64 [4] (``rollout_moments_shards``: the moments over all shards) used in place of the handle's own; together with
        ``normalize=False`` it is refused by name.
        ``unit="segment"`` (truncated segments of a recurrent policy; npb_rollout_minibatch_segments; after ``policy_segments(every)``): a
        permutation of the ``(t / every) * n`` segments; ``index`` [count] is the segment id ``c * n + p``, every tensor is time-major
        [every, count, ...] with ``out[s][j] = src[c * every + s][p]``, and the dict carries ``"every"``.  ``t % every != 0`` is refused.
        THE YIELDED TENSORS ARE VIEWS OF BUFFERS THE ENV KEEPS, the same storage on every yield: use or copy a minibatch before asking for
        the next.  ``act`` / ``extra`` are None where the rollout has none.  ``set_rollout(None)`` drops the buffers.
        ``nuclear_sim_amd.rollout.minibatch`` is the same in numpy, bit for bit."""
        ro = self._on("_roll")
        if not hasattr(self.L, "npb_rollout_minibatch"):
            raise _lib.NpbError("libnpb.so has no npb_rollout_minibatch: rebuild")
        if unit not in _lib.MINIBATCH_UNITS:
            raise ValueError("a minibatch's unit is 'transition' or 'plant', not %r (or 'segment', after policy_segments())" % (unit,))
        every = self._segments("rollout_minibatches(unit='segment')")["every"] if unit == "segment" else None
        B, epochs, first_epoch = int(batch_size), int(epochs), int(first_epoch)
        if B < 1 or epochs < 0:
            raise ValueError("batch_size must be >= 1 and epochs >= 0")
        if not float(eps) >= 0.0:
            raise ValueError("eps must be >= 0")
        if moments is not None:
            if not normalize:
                raise ValueError("moments= are given and normalize=False: the moments are what normalises the advantages")
            if not isinstance(moments, torch.Tensor) or moments.dtype != torch.float64 or tuple(moments.shape) != (4,) or \
                    not moments.is_contiguous() or moments.device != self.device:
                raise ValueError("moments must be a contiguous float64 [4] tensor on %s" % (self.device,))
        adv, ret, t = self._last_advantages(ro, advantages)
        if t < 1:
            raise _lib.NpbError("nothing recorded yet (t == 0)")
        plant = unit != "transition"      # (time-major outputs: whole sequences, or segments)
        slots = t if unit == "plant" else every
        if every is not None:
            if not hasattr(self.L, "npb_rollout_minibatch_segments"):
                raise _lib.NpbError("libnpb.so has no npb_rollout_minibatch_segments: rebuild")
            recurrent.chunks_of(t, every)
        N = self.n if unit == "plant" else (t * self.n if every is None else (t // every) * self.n)
        if N > rollout.N_MAX or t * self.n > rollout.N_MAX and unit != "plant":
            raise ValueError("t * n = %d is beyond 2^31 - 1, what an index holds" % N)
        B = min(B, N)
        if moments is None:
            moments = self.rollout_moments(adv[:t], ddof) if normalize else None
        spec, tensors = ro["spec"], ro["tensors"]
        (K, C), A, E = spec["stack"], spec["axes"], spec["extras"]
        rows = B * slots if plant else B
        key = (B, rows, adv.dtype)
        if ro.get("mb_key") != key:      # the buffers: one set, flat, as many rows as the largest minibatch has
            with torch.cuda.device(self.device):
                def zeros(cells, dtype):
                    return torch.zeros(rows * cells, dtype=dtype, device=self.device)
                ro["mb"] = {"index": torch.zeros(B, dtype=torch.int32, device=self.device), "obs": zeros(K * C, tensors["obs"].dtype),
                            "act": zeros(A, tensors["act"].dtype) if A else None, "extra": zeros(E, torch.float32) if E else None,
                            "adv": zeros(1, adv.dtype), "ret": zeros(1, adv.dtype)}
            ro["mb_key"] = key
        buf = ro["mb"]
        d = _lib.NpbMinibatchDesc()
        d.unit, d.type, d.eps, d.max_blocks = _lib.MINIBATCH_UNITS[unit], _lib.ROLLOUT_DTYPES[self._MB_DTYPES[adv.dtype]], float(eps), int(max_blocks)
        d.adv, d.ret, d.moments = adv.data_ptr(), ret.data_ptr(), None if moments is None else moments.data_ptr()
        d.index, d.obs, d.adv_out, d.ret_out = buf["index"].data_ptr(), buf["obs"].data_ptr(), buf["adv"].data_ptr(), buf["ret"].data_ptr()
        d.act = None if buf["act"] is None else buf["act"].data_ptr()
        d.extra = None if buf["extra"] is None else buf["extra"].data_ptr()

        def view(x, count, *cells):
            shape = ((slots, count) if plant else (count,)) + cells
            return None if x is None else x[:int(np.prod(shape))].view(shape)

        def batches():
            held = (adv, ret, moments)      # (alive while the launches read them)
            for e in range(first_epoch, first_epoch + epochs):
                d.keys[:] = [int(k) for k in rollout.permutation_keys(seed, e)]
                for first in range(0, N, B):
                    count = min(B, N - first)
                    if count < B and drop_last:
                        break
                    d.first, d.count = first, count
                    if every is None:
                        _lib.check(self.L.npb_rollout_minibatch(self._h, ctypes.byref(d), self._stream()), self._h)
                    else:
                        _lib.check(self.L.npb_rollout_minibatch_segments(self._h, ctypes.byref(d), every, self._stream()), self._h)
                    batch = {"index": buf["index"][:count], "obs": view(buf["obs"], count, K, C), "act": view(buf["act"], count, A),
                             "extra": view(buf["extra"], count, E), "adv": view(buf["adv"], count), "ret": view(buf["ret"], count), "epoch": e}
                    if every is not None:
                        batch["every"] = every
                    yield batch
            del held
        return batches()

    # ------------------------------------------------------------------ the policy on the device
    @staticmethod
    def _policy_layers(net, who):
        """a net as a list of ``(W, b)`` tensors: the ``nn.Linear`` layers of a module in their order, or the caller's pairs"""
        if isinstance(net, torch.nn.Module):
            pairs = [(m.weight, m.bias) for m in net.modules() if isinstance(m, torch.nn.Linear)]
            if any(b is None for _, b in pairs):
                raise ValueError("a Linear layer of the %s has no bias" % who)
        else:
            pairs = [(torch.as_tensor(W), torch.as_tensor(b)) for W, b in net]
        if len(pairs) < 2:
            raise ValueError("the %s needs at least one hidden layer and its head" % who)
        for W, b in pairs:
            if W.dim() != 2 or tuple(b.shape) != (W.shape[0],):
                raise ValueError("a layer of the %s is W[out][in] with b[out]" % who)
        return pairs

    @staticmethod
    def _policy_core(core):
        """a core as ``(W_ih, b_ih, W_hh, b_hh)`` tensors, theta's order: a ``torch.nn.GRUCell``'s parameters, or the caller's
        ``(W_ih, W_hh, b_ih, b_hh)`` (GRUCell's own order)"""
        if isinstance(core, torch.nn.GRUCell):
            if not core.bias:
                raise ValueError("the core's GRUCell has no bias")
            core = (core.weight_ih, core.weight_hh, core.bias_ih, core.bias_hh)
        if not isinstance(core, (tuple, list)) or len(core) != 4:
            raise ValueError("core is a torch.nn.GRUCell or (W_ih, W_hh, b_ih, b_hh)")
        W_ih, W_hh, b_ih, b_hh = (torch.as_tensor(v) for v in core)
        H = W_hh.shape[-1]
        if W_ih.dim() != 2 or W_ih.shape[0] != 3 * H or tuple(W_hh.shape) != (3 * H, H) or tuple(b_ih.shape) != (3 * H,) or tuple(b_hh.shape) != (3 * H,):
            raise ValueError("a core is W_ih[3H][cells], W_hh[3H][H], b_ih[3H], b_hh[3H]")
        return W_ih, b_ih, W_hh, b_hh

    def _policy_theta(self, actor, critic, log_std, core=None):
        """``(theta, actor widths, critic widths)``: theta a float32 device tensor in the statement's order, std = exp(log_std) formed here;
        ``core``: its four tensors come first (``recurrent.pack``)"""
        a, c = self._policy_layers(actor, "actor"), self._policy_layers(critic, "critic")
        g = [] if core is None else list(self._policy_core(core))
        with torch.no_grad():
            ls = torch.as_tensor(log_std).detach().to(device=self.device, dtype=torch.float32).reshape(-1)
            flat = [x.detach().to(device=self.device, dtype=torch.float32).reshape(-1) for x in g + [x for W, b in a + c for x in (W, b)]]
            theta = torch.cat(flat + [ls, torch.exp(ls)]).contiguous()
        shapes = tuple([tuple(W.shape) for W, _ in net] for net in (a, c))
        return theta, shapes, int(ls.numel())

    def set_policy(self, actor, critic=None, log_std=None, activation: str = "tanh", seed: int = 0, deterministic: bool = False, extras=None,
                   first_plant: int = 0, core=None, gates: str = "soft") -> None:
        """Run the policy on the device (npb_set_policy): in front of every ``step()`` ONE launch reads every plant's features stack,
        runs a diagonal-Gaussian actor and a critic -- two MLPs of 1 to 3 hidden layers, up to 128 wide, ``"relu"`` or ``"tanh"`` -- draws
        the noise, and writes the action into ``controls_input()``, and value and log-probability into tensors the env keeps
        (``policy_outputs()``, ``info["value"]``, ``info["logp"]``).  Features and controls must be set; the actor's head has one output
        per axis.  ``actor`` / ``critic``: ``torch.nn`` modules (their ``Linear`` layers in order, head last) or lists of ``(W, b)``;
        ``log_std``: [n_axes]; ``std = exp(log_std)`` is formed here, in torch.  ``extras``: with a rollout set, where value and logp go
        in its extras -- a tuple of names in slot order, e.g. ``("value", "logp")`` (None entries are left to the caller), or a dict
        name -> slot -- so the rollout records them by itself.  ``seed`` and ``first_plant`` key the noise (Philox4x32-10, counter
        ``(first_plant + p, t, j)``): shards of one batch draw what the whole batch would.  ``deterministic``: the mean, no draw.
        While a policy is set ``set_features``, ``set_controls`` and ``set_rollout`` are refused, and so is ``step(controls=...)``.
        ``nuclear_sim_amd.policy`` is the same in numpy: bit for bit with relu, within the float tanh's error with tanh.
        ``logp`` is the density of the unrounded action.  ``set_policy(None)`` turns it off.
        ``core``: a ``torch.nn.GRUCell`` or ``(W_ih, W_hh, b_ih, b_hh)`` -- a recurrent policy (npb_set_policy_core): the cell reads the
        features, both nets read its new hidden state (their first layers take the cell's width), and the state is carried per plant in
        ``policy_hidden()`` and restarts with the plant's episode -- the autoreset's restarts, ``reset``, ``restore`` and
        ``restore_from_bank``.  ``gates``: ``"soft"`` (GRUCell's sigmoid and tanh) or ``"hard"`` (piecewise linear, bit-exact).  With a
        rollout set, ``policy_rollout_hidden()`` has the state in front of slot 0 and the states beside ``final_obs``.
        ``nuclear_sim_amd.recurrent`` is the same in numpy.  A recurrent policy trains through time on the device, on whole sequences:
        ``policy_train(..., unit="plant")``, or ``policy_grad_sequences`` on ``rollout_minibatches(unit="plant")`` and ``policy_adam``.
        The row-wise calls (``policy_grad``, ``policy_train`` with the default unit) refuse it by name: rows carry no order."""
        if actor is None:
            if self._pol is not None:
                _lib.check(self.L.npb_set_policy(self._h, None), self._h)
            self._pol = None
            return
        ft, ct = self._on("_feat"), self._on("_ctl")
        if not hasattr(self.L, "npb_set_policy"):
            raise _lib.NpbError("libnpb.so has no npb_set_policy: rebuild")
        if critic is None or log_std is None:
            raise ValueError("set_policy takes an actor, a critic and log_std")
        theta, (ashape, cshape), n_ls = self._policy_theta(actor, critic, log_std, core)
        n, (_, K, C), A = self.n, ft["out"].shape, ct["in"].shape[1]
        hidden = tuple(tuple(o for o, _ in shape[:-1]) for shape in (ashape, cshape))
        H = None if core is None else int(self._policy_core(core)[2].shape[-1])
        if core is None:
            policy.check(K * C, A, hidden[0], hidden[1], activation)
        else:
            if not hasattr(self.L, "npb_set_policy_core"):
                raise _lib.NpbError("libnpb.so has no npb_set_policy_core: rebuild")
            recurrent.check(K * C, A, hidden[0], hidden[1], activation, H, gates)
            if self._policy_core(core)[0].shape[1] != K * C:
                raise ValueError("the core does not fit: W_ih reads %d cells, not %d" % (K * C, self._policy_core(core)[0].shape[1]))
        reads = K * C if core is None else H
        want = policy.sizes(reads, A, hidden[0], hidden[1])
        if [(i, o) for o, i in ashape] != want[0] or [(i, o) for o, i in cshape] != want[1] or n_ls != A:
            raise ValueError("the nets do not fit: both read %d cells, the actor's head and log_std have %d entries, the critic's head one" % (reads, A))
        slots = {"value": -1, "logp": -1}
        if extras is not None:
            ro = self._on("_roll")
            named = extras.items() if isinstance(extras, dict) else [(name, j) for j, name in enumerate(extras) if name is not None]
            for name, j in named:
                if name not in slots or slots[name] >= 0 or not 0 <= int(j) < ro["spec"]["extras"]:
                    raise ValueError("extras names 'value' and 'logp' once each, in slots 0 .. %d, not %r" % (ro["spec"]["extras"] - 1, extras))
                slots[name] = int(j)
        with torch.cuda.device(self.device):
            value = torch.zeros((n,), dtype=torch.float32, device=self.device)
            logp = torch.zeros((n,), dtype=torch.float32, device=self.device)
        d = _lib.NpbPolicyDesc()
        for name, widths in (("actor", hidden[0]), ("critic", hidden[1])):
            setattr(d, name + "_layers", len(widths))
            for l, w in enumerate(widths):
                getattr(d, name + "_width")[l] = w
        d.activation, d.deterministic, d.seed, d.first_plant = _lib.POLICY_ACTIVATIONS[activation], int(bool(deterministic)), int(seed) & (2 ** 64 - 1), int(first_plant)
        d.value, d.logp = value.data_ptr(), logp.data_ptr()
        d.value_slot, d.logp_slot = slots["value"], slots["logp"]
        if extras is not None and (slots["value"] >= 0 or slots["logp"] >= 0):
            d.extras_in, d.n_extras = self._roll["extras_in"].data_ptr(), self._roll["spec"]["extras"]
        cell = {}
        if core is None:
            _lib.check(self.L.npb_set_policy(self._h, ctypes.byref(d)), self._h)      # (refused: what was set before stays)
        else:
            R = 0 if self._roll is None else self._roll["spec"]["final_rows"]
            with torch.cuda.device(self.device):
                cell = {"hidden": torch.zeros((n, H), dtype=torch.float32, device=self.device),
                        "first": None if self._roll is None else torch.zeros((n, H), dtype=torch.float32, device=self.device),
                        "final": torch.zeros((n * R, H), dtype=torch.float32, device=self.device) if R else None,
                        "state": (("hidden", np.float32, (n, H)), ("seen", np.int32, (n,)), ("primed", np.int32, (n,)))}
            g = _lib.NpbPolicyCore()
            g.width, g.gates, g.hidden, g.final_rows = H, _lib.POLICY_GATES[gates], cell["hidden"].data_ptr(), R
            g.first = None if cell["first"] is None else cell["first"].data_ptr()
            g.final = None if cell["final"] is None else cell["final"].data_ptr()
            _lib.check(self.L.npb_set_policy_core(self._h, ctypes.byref(d), ctypes.byref(g)), self._h)
        self._pol = {"value": value, "logp": logp, "theta": None,
                     "spec": {"cells": K * C, "n_axes": A, "actor": hidden[0], "critic": hidden[1], "activation": activation,
                              "seed": int(seed) & (2 ** 64 - 1), "deterministic": bool(deterministic), "first_plant": int(first_plant),
                              "act_dtype": str(ct["in"].dtype).split(".")[1], "extras": dict(slots), "core": H, "gates": gates if core is not None else None}}
        self._pol.update(cell)
        self._policy_upload(theta)

    def _policy_upload(self, theta) -> None:
        pol = self._on("_pol")
        S = pol["spec"]
        takes = recurrent.theta_size(S["cells"], S["n_axes"], S["actor"], S["critic"], S["core"])
        if theta.numel() != takes:
            raise ValueError("theta has %d elements, the set policy takes %d" % (theta.numel(), takes))
        _lib.check(self.L.npb_policy_load(self._h, ctypes.c_void_p(theta.data_ptr()), 1, self._stream()), self._h)
        pol["theta"], pol["moved"] = theta, False      # (alive while the launch reads it)

    def policy_load(self, theta_or_modules) -> None:
        """New parameters into the set policy (npb_policy_load), once per optimiser iteration: a flat float32 ``theta`` in the
        statement's order (``policy.pack``), device or host, or ``(actor, critic, log_std)`` as ``set_policy`` takes them -- with a
        core the longer ``theta`` of ``recurrent.pack``, or ``(core, actor, critic, log_std)``.  No reallocation, nothing read back; the
        shapes stay."""
        has_core = self._on("_pol")["spec"]["core"] is not None
        if isinstance(theta_or_modules, (tuple, list)) and len(theta_or_modules) == 3 + has_core and not isinstance(theta_or_modules[0], (int, float)):
            parts = tuple(theta_or_modules)
            theta, _, _ = self._policy_theta(*parts[has_core:], core=parts[0] if has_core else None)
        else:
            theta = torch.as_tensor(theta_or_modules).detach().to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        self._policy_upload(theta)

    def policy_outputs(self) -> Dict[str, torch.Tensor]:
        """``value`` and ``logp``, float32 [n] each, the same storage on every call: what the policy made of the features in front of the
        last step.  The action is ``controls_input()``."""
        pol = self._on("_pol")
        return {"value": pol["value"], "logp": pol["logp"]}

    def policy_theta(self) -> torch.Tensor:
        """the handle's current parameters, a flat float32 device tensor in the statement's order (what ``policy.Policy.load`` takes): the
        tensor last loaded until ``policy_adam`` / ``policy_train`` has moved them, then a copy of the handle's (npb_policy_get_theta)"""
        pol = self._on("_pol")
        if pol.get("moved"):
            with torch.cuda.device(self.device):
                theta = torch.zeros_like(pol["theta"])
            _lib.check(self.L.npb_policy_get_theta(self._h, ctypes.c_void_p(theta.data_ptr()), self._stream()), self._h)
            pol["theta"], pol["moved"] = theta, False
        return pol["theta"]

    # ------------------------------------------------------------------ training the policy on the device
    def _ppo_desc(self, batch, clip, vf_coef, ent_coef, max_grad_norm, rows_per_chain, max_blocks=0):
        """``(descriptor, tensors kept alive)`` of one minibatch: a dict as ``rollout_minibatches`` yields (``logp_old`` from the extras
        slot the policy was set with) or one of explicit tensors ``obs``, ``act``, ``logp_old``, ``adv``, ``ret``"""
        pol = self._on("_pol")
        if not hasattr(self.L, "npb_policy_grad"):
            raise _lib.NpbError("libnpb.so has no npb_policy_grad: rebuild")
        S = pol["spec"]
        for name in ("obs", "act", "adv", "ret"):
            if batch.get(name) is None:
                raise ValueError("a minibatch needs %r" % name)
        old = batch.get("logp_old")
        if old is None:
            slot = S["extras"]["logp"]
            if batch.get("extra") is None or slot < 0:
                raise ValueError("no logp_old: pass it, or set the policy with extras naming 'logp' so the rollout records it")
            old = batch["extra"][..., slot]
        floats = (torch.float32, torch.float64)

        def dev(x, dtypes, what):
            x = torch.as_tensor(x)
            if x.dtype not in dtypes:
                raise ValueError("%s must be %s, not %r" % (what, " or ".join(str(t) for t in dtypes), x.dtype))
            return x.to(device=self.device).contiguous()
        obs, act = dev(batch["obs"], floats, "obs"), dev(batch["act"], floats, "act")
        old, adv = dev(old, (torch.float32,), "logp_old").reshape(-1), dev(batch["adv"], floats, "adv").reshape(-1)
        ret = dev(batch["ret"], (adv.dtype,), "ret").reshape(-1)
        count = adv.numel()
        if count < 1 or obs.numel() != count * S["cells"] or act.numel() != count * S["n_axes"] or old.numel() != count or ret.numel() != count:
            raise ValueError("a minibatch of %d rows takes obs of %d cells and act of %d axes a row, and logp_old and ret of its length"
                             % (count, S["cells"], S["n_axes"]))
        if str(act.dtype).split(".")[1] != S["act_dtype"]:
            raise ValueError("act must be of the controls' input type, %s" % S["act_dtype"])
        d = _lib.NpbPpoDesc()
        d.obs, d.obs_type = obs.data_ptr(), _lib.FEATURE_DTYPES[self._MB_DTYPES[obs.dtype]]
        d.act, d.act_type = act.data_ptr(), _lib.CONTROL_DTYPES[self._MB_DTYPES[act.dtype]]
        d.logp_old, d.adv, d.ret, d.adv_type, d.count = old.data_ptr(), adv.data_ptr(), ret.data_ptr(), _lib.ROLLOUT_DTYPES[self._MB_DTYPES[adv.dtype]], count
        d.clip, d.vf_coef, d.ent_coef, d.max_grad_norm = float(clip), float(vf_coef), float(ent_coef), float(max_grad_norm)
        d.rows_per_chain, d.max_blocks = int(rows_per_chain), int(max_blocks)
        return d, [obs, act, old, adv, ret]

    def _ppo_more(self, batch, count, clip_vf, value_old, kl_limit=0.0):
        """``(npb_ppo_more_t or None, tensors kept alive)``: the options of one update.  None with every option off: the caller then
        makes the plain call.  ``value_old`` defaults to the batch's extras slot the policy was set with for ``"value"``"""
        clip_vf, kl_limit = float(clip_vf), float(kl_limit)
        if not 0.0 <= clip_vf < float("inf"):
            raise ValueError("clip_vf must be finite and >= 0 (0 = off), not %r" % (clip_vf,))
        if clip_vf == 0.0 and kl_limit == 0.0:
            return None, []
        if not hasattr(self.L, "npb_policy_grad_more"):
            raise _lib.NpbError("libnpb.so has no npb_policy_grad_more: rebuild")
        m, held = _lib.NpbPpoMore(), []
        m.clip_vf, m.kl_limit = clip_vf, kl_limit
        if clip_vf > 0.0:
            if value_old is None:
                value_old = batch.get("value_old")
            if value_old is None:
                slot = self._pol["spec"]["extras"]["value"]
                if batch.get("extra") is None or slot < 0:
                    raise ValueError("clip_vf > 0 and no value_old: pass it, or set the policy with extras naming 'value' so the rollout records it")
                value_old = batch["extra"][..., slot]
            value_old = torch.as_tensor(value_old)
            if value_old.dtype != torch.float32 or value_old.numel() != count:
                raise ValueError("value_old must be float32 with one value a row (%d)" % count)
            value_old = value_old.to(device=self.device).contiguous().reshape(-1)
            m.value_old = value_old.data_ptr()
            held.append(value_old)
        return m, held

    def policy_grad(self, batch, clip: float = 0.2, vf_coef: float = 0.5, ent_coef: float = 0.0, max_grad_norm: float = 0.5,
                    rows_per_chain: int = 256, diagnostics: bool = False, max_blocks: int = 0, clip_vf: float = 0.0, value_old=None) -> dict:
        """The PPO loss of one minibatch and its gradient through both nets, on the device (npb_policy_grad): ``{"grad", "stats",
        "more"}`` -- ``grad`` float32 in theta's layout, clipped to ``max_grad_norm`` (0 = off), ``stats`` float64 [8] in ``ppo.STATS``'s
        order, ``more`` float64 [4] in ``ppo.STATS_MORE``'s, all device tensors, nothing read back -- and with ``diagnostics`` also
        ``logp_new``, ``value_new`` (float32) and ``ratio`` (float64),
        [count] each.  ``batch``: a dict as ``rollout_minibatches`` yields (``logp_old`` is the extras slot the policy was set with) or one
        with ``obs``, ``act``, ``logp_old``, ``adv``, ``ret``.  ``rows_per_chain`` pins the order of the sums over rows; no bit depends on
        ``max_blocks``.  ``clip_vf`` > 0 clips the value loss around ``value_old`` (float32 [count]; by default the batch's extras slot
        the policy was set with for ``"value"``).  ``nuclear_sim_amd.ppo.gradient`` is the same in numpy: bit for bit with relu when fed
        the device's ``ratio``."""
        return self._ppo_grad(self._ppo_request(batch, clip, vf_coef, ent_coef, max_grad_norm, rows_per_chain, max_blocks, clip_vf, value_old), diagnostics)

    def _ppo_request(self, batch, clip, vf_coef, ent_coef, max_grad_norm, per_chain, max_blocks=0, clip_vf=0.0, value_old=None, kl_limit=0.0, sequences=False,
                     what="training through time"):
        """THE REQUEST of one minibatch, what every training call below hands to ``_ppo_call``: ``d`` (``_ppo_desc``), ``more``
        (``_ppo_more``; None with every option off), ``seq`` and ``seg`` (``_ppo_seq``; None for rows, ``seg`` None for whole
        sequences) and ``held``, the ONE list of every tensor a descriptor points into: whoever launches keeps that list.
        ``sequences``: a minibatch of sequences or segments, not of rows; ``what``: the caller's name in the refusal of a policy without a core"""
        d, held = self._ppo_desc(batch, clip, vf_coef, ent_coef, max_grad_norm, per_chain, max_blocks)
        more, held_more = self._ppo_more(batch, d.count, clip_vf, value_old, kl_limit)
        seq = seg = None
        if sequences:
            self._policy_cell(what)
            seq, seg, held_seq = self._ppo_seq(batch, d)
            held_more = held_more + held_seq
        return {"d": d, "more": more, "seq": seq, "seg": seg, "held": held + held_more}

    def _ppo_call(self, op, req, *tail) -> None:
        """THE ONE MAP from (operation, kind) to the entry point: ``op`` is ``"grad"``, ``"update"`` or ``"shard_sums"``; the kind is the
        request's -- rows (the plain / ``_more`` split of ``grad`` and ``update`` lives here), whole sequences (``_seq``) or segments
        (``_segments``).  ``tail``: the operation's own arguments behind the descriptors.  The request's tensors stay alive on the env
        while the launches read them"""
        d, more, seq, seg = (None if req[k] is None else ctypes.byref(req[k]) for k in ("d", "more", "seq", "seg"))
        if seq is not None:
            name, args = "npb_policy_%s_%s" % (op, "seq" if seg is None else "segments"), [more, seq] + ([] if seg is None else [seg])
        elif op == "shard_sums" or more is not None:
            name, args = "npb_policy_" + op + ("" if op == "shard_sums" else "_more"), [more]
        else:
            name, args = "npb_policy_" + op, []
        _lib.check(getattr(self.L, name)(self._h, d, *args, *tail, self._stream()), self._h)
        self._pol["ppo_held"] = req["held"]

    def _ppo_outputs(self, names=("grad", "stats", "more")) -> dict:
        """what the last gradient, update or combine left on the handle, copied on the stream into fresh device tensors (npb_policy_get_grad,
        _get_stats, _get_stats_more): nothing read back"""
        sizes = {"grad": (self._pol["theta"].numel(), torch.float32, "npb_policy_get_grad"), "stats": (_lib.PPO_STATS, torch.float64, "npb_policy_get_stats"),
                 "more": (_lib.PPO_STATS_MORE, torch.float64, "npb_policy_get_stats_more")}
        out = {}
        for name in names:
            count, dtype, getter = sizes[name]
            if hasattr(self.L, getter):
                with torch.cuda.device(self.device):
                    out[name] = torch.zeros(count, dtype=dtype, device=self.device)
                _lib.check(getattr(self.L, getter)(self._h, ctypes.c_void_p(out[name].data_ptr()), self._stream()), self._h)
        return out

    def _ppo_grad(self, req, diagnostics) -> dict:
        """the gradient of a request, rows or sequences: the diagnostics' tensors in the minibatch's own shape, the call, the outputs"""
        d, seq = req["d"], req["seq"]
        shape = (d.count,) if seq is None else (seq.t, seq.plants)
        out = {}
        if diagnostics:
            with torch.cuda.device(self.device):
                out = {"logp_new": torch.zeros(shape, dtype=torch.float32, device=self.device), "value_new": torch.zeros(shape, dtype=torch.float32, device=self.device),
                       "ratio": torch.zeros(shape, dtype=torch.float64, device=self.device)}
                if seq is not None:
                    out["hidden"] = torch.zeros(shape + (self._pol["spec"]["core"],), dtype=torch.float32, device=self.device)
                    seq.hidden = out["hidden"].data_ptr()
            d.logp_new, d.value_new, d.ratio = out["logp_new"].data_ptr(), out["value_new"].data_ptr(), out["ratio"].data_ptr()
        self._ppo_call("grad", req)
        out.update(self._ppo_outputs())
        return out

    def _ppo_shard_sums(self, batch, count_total, clip, vf_coef, per_chain, clip_vf, value_old, out, max_blocks, sequences) -> torch.Tensor:
        """a shard's sums of a minibatch of rows or of sequences into ``out``, a fresh row where the caller brings none"""
        L = self.policy_shard_size()
        req = self._ppo_request(batch, clip, vf_coef, 0.0, 0.0, per_chain, max_blocks, clip_vf, value_old, sequences=sequences)
        if out is None:
            with torch.cuda.device(self.device):
                out = torch.zeros(L, dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or out.numel() != L or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous float64 tensor of %d elements on %s" % (L, self.device))
        self._ppo_call("shard_sums", req, int(count_total), ctypes.c_void_p(out.data_ptr()))
        return out

    def policy_adam(self, lr: float = 3e-4, betas=(0.9, 0.999), eps: float = 1e-5) -> None:
        """One Adam step from the gradient the last ``policy_grad`` left on the handle (npb_policy_adam): the parameters, ``std`` and the
        weights as the step reads them are refreshed on the device; ``nuclear_sim_amd.ppo.adam`` is the same in numpy"""
        pol = self._on("_pol")
        _lib.check(self.L.npb_policy_adam(self._h, float(lr), float(betas[0]), float(betas[1]), float(eps), self._stream()), self._h)
        pol["moved"] = True

    # ------------------------------------------------------------------ one policy across shards
    def policy_shard_size(self) -> int:
        """L, the length of a shard's vector for the set policy (npb_ppo_shard_count; ``ppo.shard_size``)"""
        pol = self._on("_pol")
        if not hasattr(self.L, "npb_policy_shard_sums"):
            raise _lib.NpbError("libnpb.so has no npb_policy_shard_sums: rebuild")
        return int(self.L.npb_ppo_shard_count(pol["theta"].numel(), pol["spec"]["n_axes"]))

    def policy_shard_sums(self, batch, count_total: int, clip: float = 0.2, vf_coef: float = 0.5, rows_per_chain: int = 256,
                          clip_vf: float = 0.0, value_old=None, out=None, max_blocks: int = 0) -> torch.Tensor:
        """This shard's pinned double sums of one update over ``count_total`` rows in all (npb_policy_shard_sums): a device float64 [L]
        -- the chains' sums of every weight and bias, not narrowed, and the 18 per-row sums, every seed divided by ``count_total`` --
        nothing read back.  ``out``: a caller's contiguous float64 [L] row to write into (a row of a [W, L] buffer: that is how one
        handle accumulates several minibatches into one Adam step).  The handle's gradient and statistics are left as they were.
        ``nuclear_sim_amd.ppo.shard_sums`` is the same in numpy: bit for bit with relu when fed the device's ``ratio``."""
        return self._ppo_shard_sums(batch, count_total, clip, vf_coef, rows_per_chain, clip_vf, value_old, out, max_blocks, False)

    def _ppo_shards(self, shards, count_total, ent_coef, max_grad_norm, kl_limit=0.0):
        """the npb_ppo_shards_t of a contiguous device float64 [W, L] tensor"""
        L = self.policy_shard_size()
        if not isinstance(shards, torch.Tensor) or shards.dtype != torch.float64 or shards.dim() != 2 or shards.shape[1] != L or \
                not shards.is_contiguous() or shards.device != self.device:
            raise ValueError("shards must be a contiguous float64 [W, %d] tensor on %s" % (L, self.device))
        s = _lib.NpbPpoShards()
        s.sums, s.n_shards, s.count_total = shards.data_ptr(), shards.shape[0], int(count_total)
        s.ent_coef, s.max_grad_norm, s.kl_limit = float(ent_coef), float(max_grad_norm), float(kl_limit)
        return s

    def policy_apply_shards(self, shards, count_total: int, ent_coef: float = 0.0, max_grad_norm: float = 0.5, lr: float = 3e-4,
                            betas=(0.9, 0.999), eps: float = 1e-5, kl_limit: float = 0.0) -> None:
        """One update from W shards' vectors (npb_policy_apply_shards): ``shards`` a contiguous device float64 [W, L] in shard order, added
        in ascending order in double, narrowed once, clipped, then the Adam step; statistics with ``count = count_total`` stay on the
        handle.  Every replica that applies the same vectors computes the same bits.  ``kl_limit`` > 0: the gate on the global
        ``approx_kl``, only between npb_policy_train_begin and npb_policy_train_end.  ``ppo.combine`` and ``ppo.adam`` are the same in numpy."""
        pol = self._on("_pol")
        s = self._ppo_shards(shards, count_total, ent_coef, max_grad_norm, kl_limit)
        _lib.check(self.L.npb_policy_apply_shards(self._h, ctypes.byref(s), float(lr), float(betas[0]), float(betas[1]), float(eps), self._stream()), self._h)
        pol["moved"], pol["shards_held"] = True, shards

    def policy_combine_shards(self, shards, count_total: int, ent_coef: float = 0.0, max_grad_norm: float = 0.5) -> dict:
        """``policy_apply_shards`` without the Adam step and without a gate (npb_policy_combine_shards): ``{"grad", "stats", "more"}`` as
        ``policy_grad`` returns them, device tensors, nothing read back"""
        pol = self._on("_pol")
        s = self._ppo_shards(shards, count_total, ent_coef, max_grad_norm)
        _lib.check(self.L.npb_policy_combine_shards(self._h, ctypes.byref(s), self._stream()), self._h)
        pol["shards_held"] = shards
        return self._ppo_outputs()

    # ------------------------------------------------------------------ training through time
    def _ppo_seq(self, batch, d):
        """``(npb_ppo_seq_t, npb_ppo_segments_t or None, tensors kept alive)`` of a ``unit="plant"`` minibatch whose descriptor ``d`` is made (its ``rows_per_chain``
        counting the plants of a chain): its [t, count] shape, its
        ``index``, and the rollout's ``episode`` and ``ended`` and the core's ``first`` from the handle -- or the batch's own ``episode``
        [T, n], ``ended`` [T, n] and ``first`` [n, H], which ``index`` (None = identity) then points into.
        A SEGMENT minibatch (the batch carries ``"every"``: ``rollout_minibatches(unit="segment")``) is the same with ``t = every``, its
        sequences segments and ``index`` their ids ``c * n + p``; ``first`` is then the stored states [chunks, n, H] (the handle's: what
        ``policy_segments`` bound, its first ``recorded slots / every`` rows), and the second member is the
        npb_ppo_segments_t that selects the segment entry points (None for whole sequences)"""
        pol = self._policy_cell("training through time")
        if not hasattr(self.L, "npb_policy_grad_seq"):
            raise _lib.NpbError("libnpb.so has no npb_policy_grad_seq: rebuild")
        H = pol["spec"]["core"]
        shape = tuple(torch.as_tensor(batch["adv"]).shape)
        if len(shape) != 2:
            raise ValueError("a sequence minibatch is time-major, adv [t, count] (rollout_minibatches(unit='plant')), not %r" % (shape,))
        t, count = shape
        every = batch.get("every")
        if every is not None:
            if not hasattr(self.L, "npb_policy_grad_segments"):
                raise _lib.NpbError("libnpb.so has no npb_policy_grad_segments: rebuild")
            if int(every) != t:
                raise ValueError("a segment minibatch is [every, count]: every = %r, and adv has %d slots" % (every, t))
        own = [batch.get(name) for name in ("episode", "ended", "first")]
        if any(x is None for x in own):
            if any(x is not None for x in own):
                raise ValueError("episode, ended and first come together: all three, or none (the rollout's)")
            ro = self._on("_roll")
            if pol["first"] is None:
                raise _lib.NpbError("the policy was set without a rollout (set_rollout, then set_policy): no state in front of slot 0")
            own = [ro["tensors"]["episode"], ro["tensors"]["ended"], pol["first"]]
            if every is not None:
                seg = self._segments("a segment minibatch without its own episode, ended and first")
                if seg["every"] != t:
                    raise ValueError("the batch's every = %d is not policy_segments' %d" % (t, seg["every"]))
                recorded = int(self.L.npb_rollout_steps(self._h))
                own[2] = seg["starts"][:recurrent.chunks_of(recorded, t)]
        episode, ended, first = (torch.as_tensor(x).to(device=self.device).contiguous() for x in own)
        if episode.dtype != torch.int32 or ended.dtype != torch.uint8 or first.dtype != torch.float32:
            raise ValueError("episode is int32, ended uint8 and first float32")
        chunks = None
        if every is not None:
            if first.dim() != 3 or first.shape[2] != H or episode.dim() != 2 or episode.shape[1] != first.shape[1] or \
                    episode.shape[0] < first.shape[0] * t or ended.shape != episode.shape:
                raise ValueError("a segment minibatch's first is the stored states [chunks, n, %d], episode and ended [>= chunks * %d, n]" % (H, t))
            chunks, n = first.shape[0], first.shape[1]
        else:
            n = first.shape[0]
            if first.dim() != 2 or first.shape[1] != H or episode.dim() != 2 or episode.shape[1] != n or episode.shape[0] < t or ended.shape != episode.shape:
                raise ValueError("episode and ended are [>= %d, n] and first [n, %d]" % (t, H))
        index = batch.get("index")
        if index is None and count != n * (chunks or 1):
            raise ValueError("a minibatch of %d of the rollout's %d %s needs its index" % (count, n * (chunks or 1), "plants" if chunks is None else "segments"))
        held = [episode, ended, first]
        s = _lib.NpbPpoSeq()
        seg = None
        if chunks is not None:
            seg = _lib.NpbPpoSegments()
            seg.every, seg.chunks = t, chunks
        s.t, s.plants, s.n_plants = t, count, n
        s.episode, s.ended, s.first = episode.data_ptr(), ended.data_ptr(), first.data_ptr()
        if index is not None:
            index = torch.as_tensor(index).to(device=self.device).contiguous()
            if index.dtype != torch.int32 or index.numel() != count:
                raise ValueError("index must be int32 with one entry a sequence (%d)" % count)
            s.index = index.data_ptr()
            held.append(index)
        return s, seg, held

    def policy_grad_sequences(self, batch, clip: float = 0.2, vf_coef: float = 0.5, ent_coef: float = 0.0, max_grad_norm: float = 0.5,
                              plants_per_chain: int = 32, diagnostics: bool = False, max_blocks: int = 0, clip_vf: float = 0.0, value_old=None) -> dict:
        """``policy_grad`` for a policy with a core (npb_policy_grad_seq): the PPO loss of one minibatch of WHOLE SEQUENCES and its
        gradient through both nets, through the cell and through time, on the device.  ``batch``: as ``rollout_minibatches(unit="plant")``
        yields it, every tensor time-major [t, count, ...]; the restart words and the state in front of slot 0 are the handle's own
        (the rollout's ``episode`` and ``ended``, ``policy_rollout_hidden()["first"]``), read through the batch's ``index`` -- or the
        batch's own ``episode``, ``ended`` and ``first``.  Returns ``{"grad", "stats", "more"}`` as ``policy_grad`` does, and with
        ``diagnostics`` ``logp_new``, ``value_new``, ``ratio`` [t, count] and ``hidden`` [t, count, H], the states under the current
        parameters.  ``plants_per_chain`` (a positive multiple of 32) pins the order of the sums; no bit depends on ``max_blocks``.
        ``first`` is the state the collecting parameters produced: after the first update of an iteration it is stale, as in every
        recurrent PPO.  ``nuclear_sim_amd.recurrent.gradient`` is the same in numpy: bit for bit with hard gates and relu when fed the
        device's ``ratio``.
        A SEGMENT minibatch (``rollout_minibatches(unit="segment")``; its ``"every"`` selects npb_policy_grad_segments) is truncated
        back-propagation through time: every sequence is one segment, started from the stored state of ``policy_segments`` (or the
        batch's own ``first`` = starts [chunks, n, H]) and differentiated within itself only; ``plants_per_chain`` counts segments.
        ``nuclear_sim_amd.recurrent.gradient_segments`` is the same in numpy."""
        return self._ppo_grad(self._ppo_request(batch, clip, vf_coef, ent_coef, max_grad_norm, plants_per_chain, max_blocks, clip_vf, value_old,
                                                sequences=True, what="policy_grad_sequences()"), diagnostics)

    def policy_shard_sums_sequences(self, batch, count_total: int, clip: float = 0.2, vf_coef: float = 0.5, plants_per_chain: int = 32,
                                    clip_vf: float = 0.0, value_old=None, out=None, max_blocks: int = 0) -> torch.Tensor:
        """``policy_shard_sums`` for a policy with a core (npb_policy_shard_sums_seq): this shard's pinned double sums of one update
        over ``count_total`` CELLS (t * plants of every shard) from a ``unit="plant"`` minibatch; ``policy_apply_shards`` and
        ``policy_combine_shards`` take the vectors.  ``nuclear_sim_amd.recurrent.shard_sums`` is the same in numpy."""
        return self._ppo_shard_sums(batch, count_total, clip, vf_coef, plants_per_chain, clip_vf, value_old, out, max_blocks, True)

    def _shard_units(self, unit, seg_every, advantages):
        """``(units, cells a unit)``: the units of this shard that ``rollout_minibatches`` cuts into minibatches -- plants of t cells each,
        recorded cells, or segments of ``seg_every`` cells each"""
        t = self._last_advantages(self._on("_roll"), advantages)[2]
        if unit == "plant":
            return self.n, t
        return (t * self.n, 1) if seg_every is None else (recurrent.chunks_of(t, seg_every) * self.n, seg_every)

    @staticmethod
    def _update_counts(cells, batch_size, epochs, drop_last):
        """the rows of every update of one shard of ``cells`` cells, as ``rollout_minibatches`` cuts them"""
        B = min(int(batch_size), int(cells))
        one = [min(B, cells - first) for first in range(0, cells, B)]
        if drop_last:
            one = [c for c in one if c == B]
        return one * int(epochs)

    def policy_train(self, batch_size, epochs: int = 1, seed: int = 0, clip: float = 0.2, vf_coef: float = 0.5, ent_coef: float = 0.0,
                     max_grad_norm: float = 0.5, rows_per_chain: Optional[int] = None, lr=3e-4, betas=(0.9, 0.999), eps: float = 1e-5,
                     clip_vf: float = 0.0, target_kl=None, more: bool = False, exchange=None, shard_cells=None, global_moments: bool = False,
                     refresh=None, **minibatches):
        """The optimiser's half of a PPO iteration: ``rollout_minibatches(batch_size, epochs, seed, **minibatches)`` and one
        npb_policy_update -- gradient and Adam step -- per minibatch.  Returns every update's stats as ONE device tensor [updates, 8]
        (``ppo.STATS``'s order), and with ``more=True`` ``(stats, more [updates, 4])`` (``ppo.STATS_MORE``'s order).  ``collect``,
        ``rollout_advantages``, ``policy_train`` is a whole iteration.
        ``lr``: a float, a sequence with one value per update, or a callable ``lr(i, updates)``: a schedule is host arithmetic.
        ``clip_vf`` > 0 clips the value loss around the values the rollout recorded (the policy's ``"value"`` extras slot).
        ``target_kl``: SB3's early stop, taken on the device: the first update whose ``approx_kl`` exceeds ``1.5 * target_kl``, and every
        later one of this call, is formed and reported but not applied; Adam's step counts the applied ones.
        With ``target_kl=None`` there is no host synchronisation.  With it set the call ends with exactly ONE stream-synchronising
        read-back, of the count of applied updates (npb_policy_train_end) -- one per iteration, none per update -- so a checkpoint taken
        after this call returns sees the right step.
        ONE POLICY ACROSS SHARDS (``exchange`` and ``shard_cells``, both or neither; with neither the call is what it was).
        ``shard_cells``: the number of recorded cells (t * n; plants for ``unit="plant"``) of every shard, in shard order, this env's
        among them (``sharding.gather_cells``).  ``exchange(vec)``: takes this shard's device float64 [L] and returns the [W, L] of all
        of them, on the device, in shard order (``sharding.ppo_exchange``).  ``batch_size`` is per shard and the advantages are
        normalised per shard -- unless ``global_moments=True``, which needs ``exchange``: ``rollout_moments_shards(exchange)`` is formed
        once, over all shards, and every minibatch of every shard is normalised with it (two exchanges of a [2] vector more, nothing
        read back).  Every shard's update count under ``batch_size`` and ``drop_last`` is formed on the host before any
        device work, and a mismatch is refused by name; update i's ``count_total`` is the sum of the shards' rows of update i, and the
        update is ``policy_shard_sums``, ``exchange``, ``policy_apply_shards``: every shard ends with the same parameters, bit for bit,
        with no broadcast.  The gate is taken on the global ``approx_kl``; the stats are the whole update's.
        A POLICY WITH A CORE trains through time with ``unit="plant"``: every minibatch is whole sequences and an update is
        npb_policy_update_seq (``policy_grad_sequences`` and the Adam step); ``rows_per_chain`` then counts the PLANTS of a chain (default
        32; row-wise a chain is 256 rows by default), and every option above works as it does row-wise.  With the default unit a policy with a core is refused
        by name: rows carry no order.
        ``unit="segment"`` (after ``policy_segments(every)``) trains over truncated segments: every minibatch is segments of ``every``
        slots and an update is npb_policy_update_segments; ``rows_per_chain`` counts SEGMENTS (default 32), ``shard_cells`` counts segments
        (``(t / every) * n``) and ``count_total`` counts cells.  ``refresh="epoch"``: ``policy_refresh_segments()`` runs before every
        epoch after the first, so the segments of later epochs start from states of the current parameters (None: they stay as
        collected)."""
        pol = self._on("_pol")
        unit = minibatches.get("unit", "transition")
        if refresh not in (None, "epoch"):
            raise ValueError("refresh is None or 'epoch', not %r" % (refresh,))
        if refresh is not None and unit != "segment":
            raise ValueError("refresh='epoch' recomputes the stored segment states: it goes with unit='segment'")
        sequences = pol["spec"]["core"] is not None and unit in ("plant", "segment")
        seg_every = self._segments("policy_train(unit='segment')")["every"] if unit == "segment" else None
        if rows_per_chain is None:      # (a chain of sequences counts plants: one tile of them; a chain of rows is 256 rows, as it was)
            rows_per_chain = 32 if sequences else 256
        kl_limit = 0.0
        if target_kl is not None:
            if not float(target_kl) > 0.0 or float(target_kl) == float("inf"):
                raise ValueError("target_kl must be finite and > 0 (None = off), not %r" % (target_kl,))
            kl_limit = 1.5 * float(target_kl)
        totals = None
        if (exchange is None) != (shard_cells is None):
            raise ValueError("exchange and shard_cells come together: both, or neither")
        if exchange is not None:
            cells = [int(c) for c in shard_cells]
            if not 1 <= len(cells) <= _lib.PPO_SHARDS_MAX or min(cells) < 1:
                raise ValueError("shard_cells: 1 .. %d shards of >= 1 cells each, not %r" % (_lib.PPO_SHARDS_MAX, cells))
            counts = [self._update_counts(c, batch_size, epochs, bool(minibatches.get("drop_last"))) for c in cells]
            if len({len(c) for c in counts}) != 1:
                raise ValueError("shard_cells: the shards make different numbers of updates (%r) under batch_size %d: shards with different "
                                 "numbers of updates are not supported" % ([len(c) for c in counts], int(batch_size)))
            own, per = self._shard_units(unit, seg_every, minibatches.get("advantages"))      # (the shards record in lockstep: one `per` for all)
            if own not in cells:
                raise ValueError("shard_cells %r does not hold this shard's own %d cells" % (cells, own))
            totals = [per * sum(c[i] for c in counts) for i in range(len(counts[0]))]
        if global_moments:
            if exchange is None:
                raise ValueError("global_moments=True needs exchange= and shard_cells=: the moments are formed over all shards")
            if minibatches.get("moments") is not None or minibatches.get("normalize", True) is False:
                raise ValueError("global_moments=True forms the moments itself: leave moments= and normalize= alone")
            adv, _, t = self._last_advantages(self._on("_roll"), minibatches.get("advantages"))
            minibatches = dict(minibatches, moments=self.rollout_moments_shards(exchange, adv[:t], minibatches.get("ddof", 1)))
        batches = self.rollout_minibatches(batch_size, epochs, seed, **minibatches)
        rates = None
        if callable(lr) or isinstance(lr, (list, tuple, np.ndarray)):
            # the number of updates, as rollout_minibatches cuts them (its batches are views of one buffer: they cannot be listed first)
            N = self._shard_units(unit, seg_every, minibatches.get("advantages"))[0]
            updates = len(self._update_counts(N, batch_size, epochs, bool(minibatches.get("drop_last"))))
            rates = [float(lr(i, updates)) for i in range(updates)] if callable(lr) else [float(x) for x in lr]
            if len(rates) != updates:
                raise ValueError("lr has %d values and the call makes %d updates" % (len(rates), updates))
        rows, mores = [], []
        b1, b2, eps = float(betas[0]), float(betas[1]), float(eps)
        if kl_limit:
            if not hasattr(self.L, "npb_policy_train_begin"):
                raise _lib.NpbError("libnpb.so has no npb_policy_train_begin: rebuild")
            _lib.check(self.L.npb_policy_train_begin(self._h, self._stream()), self._h)
        try:
            epoch0 = None
            for i, batch in enumerate(batches):
                if refresh is not None:      # (the batch is gathered already: the gather reads no stored state)
                    epoch0 = batch["epoch"] if epoch0 is None else epoch0
                    if batch["epoch"] != epoch0:
                        epoch0 = batch["epoch"]
                        self.policy_refresh_segments()
                rate = float(lr) if rates is None else rates[i]
                if totals is None:
                    self._ppo_call("update", self._ppo_request(batch, clip, vf_coef, ent_coef, max_grad_norm, rows_per_chain, 0, clip_vf, None, kl_limit, sequences),
                                   rate, b1, b2, eps)
                else:
                    vec = self._ppo_shard_sums(batch, totals[i], clip, vf_coef, rows_per_chain, clip_vf, None, None, 0, sequences)
                    pol["ppo_held"] = pol["ppo_held"] + [vec]
                    every = exchange(vec)
                    if not isinstance(every, torch.Tensor) or every.shape != (len(cells), vec.numel()):
                        raise ValueError("exchange must return the [%d, %d] tensor of every shard's sums" % (len(cells), vec.numel()))
                    self.policy_apply_shards(every.contiguous(), totals[i], ent_coef, max_grad_norm, rate, (b1, b2), eps, kl_limit)
                got = self._ppo_outputs(("stats", "more") if more else ("stats",))
                pol["moved"] = True
                rows.append(got["stats"])
                if more:
                    mores.append(got["more"])
        finally:
            if kl_limit:      # (the one read-back; and whatever was refused above, nothing stays armed)
                applied = ctypes.c_uint32()
                _lib.check(self.L.npb_policy_train_end(self._h, ctypes.byref(applied), self._stream()), self._h)
        with torch.cuda.device(self.device):
            stats = torch.stack(rows) if rows else torch.zeros((0, _lib.PPO_STATS), dtype=torch.float64, device=self.device)
            if not more:
                return stats
            return stats, (torch.stack(mores) if mores else torch.zeros((0, _lib.PPO_STATS_MORE), dtype=torch.float64, device=self.device))

    def policy_optimizer_state(self) -> Dict[str, np.ndarray]:
        """Adam's state for a checkpoint (npb_policy_optimizer_get_state): ``m``, ``v`` float32 in theta's layout, and ``step``"""
        pol = self._on("_pol")
        m, v = (np.zeros(pol["theta"].numel(), dtype=np.float32) for _ in range(2))
        step = ctypes.c_uint64()
        _lib.check(self.L.npb_policy_optimizer_get_state(self._h, m.ctypes.data, v.ctypes.data, ctypes.byref(step), self._stream()), self._h)
        return {"m": m, "v": v, "step": np.uint64(step.value)}

    def load_policy_optimizer_state(self, state) -> None:
        """put back what ``policy_optimizer_state()`` returned (npb_policy_optimizer_set_state)"""
        pol = self._on("_pol")
        m, v = (np.ascontiguousarray(state[k], dtype=np.float32).reshape(-1) for k in ("m", "v"))
        if m.size != pol["theta"].numel() or v.size != m.size:
            raise ValueError("m and v have theta's %d elements" % pol["theta"].numel())
        _lib.check(self.L.npb_policy_optimizer_set_state(self._h, m.ctypes.data, v.ctypes.data, int(state["step"]), self._stream()), self._h)

    def _policy_cell(self, what) -> dict:
        pol = self._on("_pol")
        if pol["spec"]["core"] is None:
            raise _lib.NpbError("%s: the policy has no core (set_policy(core=...))" % what)
        return pol

    def policy_hidden(self) -> torch.Tensor:
        """The recurrent policy's live hidden state, float32 [n, H], the same storage on every call: what the cell made of the features in
        front of the last step.  A restarted plant's row is read as zeros by the next step; the row itself stays until then."""
        return self._policy_cell("policy_hidden()")["hidden"]

    def policy_rollout_hidden(self) -> Dict[str, torch.Tensor]:
        """What a recurrent policy records beside a rollout: ``first`` float32 [n, H], the state the policy read in front of slot 0 (the
        restart rule applied), from which ``recurrent.replay`` forms the state in front of every slot; ``final`` float32
        [n * final_rows, H], the states beside ``final_obs``: ``policy_values(final_obs, hidden=final)`` are the ``final_values``."""
        pol = self._policy_cell("policy_rollout_hidden()")
        self._on("_roll")
        if pol["first"] is None:
            raise _lib.NpbError("policy_rollout_hidden(): the policy was set without a rollout (set_rollout, then set_policy)")
        H = pol["spec"]["core"]
        with torch.cuda.device(self.device):
            final = pol["final"] if pol["final"] is not None else torch.zeros((0, H), dtype=torch.float32, device=self.device)
        out = {"first": pol["first"], "final": final}
        if pol.get("segments") is not None:
            out["starts"], out["every"] = pol["segments"]["starts"], pol["segments"]["every"]
        return out

    # ------------------------------------------------------------------ truncated segments
    def _segments(self, what) -> dict:
        pol = self._policy_cell(what)
        if pol.get("segments") is None:
            raise _lib.NpbError("%s: no stored segment states (policy_segments(every) first)" % what)
        return pol["segments"]

    def policy_segments(self, every) -> None:
        """Truncated back-propagation through time for a policy with a core (npb_policy_core_segments): while collecting, the state the
        policy read in front of every slot ``c * every`` of the rollout, the restart rule applied, is kept in ``starts`` float32
        [ceil(T / every), n, H] (``policy_rollout_hidden()["starts"]``; row 0 has ``first``'s bits; rows of slots not reached keep what
        they held).  Call it after ``set_rollout`` and ``set_policy(core=...)``; ``None`` clears it; ``set_policy`` drops it.
        ``rollout_minibatches(unit="segment")`` then cuts the recorded slots into segments of ``every`` slots, ``policy_grad_sequences``
        differentiates each within itself from its stored state, ``policy_train(unit="segment")`` is the loop, and
        ``policy_refresh_segments()`` recomputes the stored states under the current parameters.  ``recurrent.starts`` is the numpy
        statement.  A handle that never calls this behaves as before."""
        if not hasattr(self.L, "npb_policy_core_segments"):
            raise _lib.NpbError("libnpb.so has no npb_policy_core_segments: rebuild")
        if every is None:
            pol = self._on("_pol")
            _lib.check(self.L.npb_policy_core_segments(self._h, 0, None, 0), self._h)
            pol.pop("segments", None)
            return
        pol = self._policy_cell("policy_segments()")
        ro = self._on("_roll")
        if pol["first"] is None:
            raise _lib.NpbError("policy_segments(): the policy was set without a rollout (set_rollout, then set_policy)")
        L, T, H = int(every), int(ro["spec"]["horizon"]), pol["spec"]["core"]
        if L < 1 or L > T:
            raise ValueError("every must be 1 .. the rollout's horizon %d, not %r" % (T, every))
        rows = -(-T // L)
        with torch.cuda.device(self.device):
            starts = torch.zeros((rows, self.n, H), dtype=torch.float32, device=self.device)
        _lib.check(self.L.npb_policy_core_segments(self._h, L, ctypes.c_void_p(starts.data_ptr()), rows), self._h)
        pol["segments"] = {"every": L, "starts": starts}

    def policy_refresh_segments(self) -> None:
        """Recompute the stored segment states under the CURRENT parameters (npb_policy_segment_starts): one forward-only launch over the
        rollout's recorded slots from ``first``; rows ``1 .. t / every - 1`` of ``starts`` are rewritten, row 0 is left alone.  Before
        any update it reproduces the recorded rows bit for bit.  ``recurrent.starts`` under the new theta is the same in numpy."""
        seg = self._segments("policy_refresh_segments()")
        self._on("_roll")
        _lib.check(self.L.npb_policy_segment_starts(self._h, seg["every"], self._stream()), self._h)

    def policy_values(self, x=None, hidden=None) -> torch.Tensor:
        """The critic alone (npb_policy_values): float32 [rows] of ``x``, a float32 or float64 device tensor [rows, K, C] (or [rows, K * C]);
        None: the current features -- the ``last_value`` of ``rollout_advantages``; the rollout's ``final_obs`` gives its ``final_values``.
        With a core (npb_policy_values_hidden) the critic reads GRU(x, hidden): ``hidden`` float32 [rows, H], the states in front of the
        rows, is required with rows of the caller's; with ``x=None`` the live hidden state is used under the restart rule."""
        pol = self._on("_pol")
        H = pol["spec"]["core"]
        if hidden is not None:
            self._policy_cell("policy_values(hidden=...)")
            if x is None:
                raise ValueError("policy_values(hidden=...) goes with rows x; x=None reads the live hidden state")
        elif H is not None and x is not None:
            raise ValueError("policy_values(x) of a recurrent policy needs hidden=, the states in front of the rows")
        own = x is None
        if x is None:
            x = self.features()
        x = torch.as_tensor(x)
        if x.dtype not in (torch.float32, torch.float64):
            raise ValueError("policy_values takes float32 or float64 rows, not %r" % (x.dtype,))
        x = x.to(device=self.device).contiguous()
        rows = x.shape[0]
        if x.numel() != rows * pol["spec"]["cells"]:
            raise ValueError("policy_values takes rows of %d cells, not %r" % (pol["spec"]["cells"], tuple(x.shape)))
        with torch.cuda.device(self.device):
            out = torch.zeros((rows,), dtype=torch.float32, device=self.device)
        ftype = _lib.FEATURE_DTYPES["float64" if x.dtype == torch.float64 else "float32"]
        if H is not None:
            if not own:
                hidden = torch.as_tensor(hidden).to(device=self.device, dtype=torch.float32).contiguous()
                if tuple(hidden.shape) != (rows, H):
                    raise ValueError("hidden is [%d, %d], one state in front of every row, not %r" % (rows, H, tuple(hidden.shape)))
            if rows:
                _lib.check(self.L.npb_policy_values_hidden(self._h, None if own else ctypes.c_void_p(x.data_ptr()), ftype, rows,
                                                           None if own else ctypes.c_void_p(hidden.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                                           self._stream()), self._h)
            pol["held"] = (x, hidden)
            return out
        if rows:
            _lib.check(self.L.npb_policy_values(self._h, ctypes.c_void_p(x.data_ptr()), ftype, rows, ctypes.c_void_p(out.data_ptr()), self._stream()), self._h)
        pol["held"] = x      # (alive while the launch reads it)
        return out

    def policy_noise(self, t: int, words: bool = False):
        """The z of draw ``t`` (npb_policy_noise), float64 [n, n_axes], by the device function the step's launch inlines; ``words``: also
        the Philox words behind it, int64-held uint32 [n, ceil(n_axes / 2), 4]"""
        A = self._on("_pol")["spec"]["n_axes"]
        with torch.cuda.device(self.device):
            z = torch.zeros((self.n, A), dtype=torch.float64, device=self.device)
            w = torch.zeros((self.n, (A + 1) // 2, 4), dtype=torch.int32, device=self.device) if words else None
        _lib.check(self.L.npb_policy_noise(self._h, int(t) & (2 ** 64 - 1), ctypes.c_void_p(z.data_ptr()), self._p(w), self._stream()), self._h)
        return (z, w.to(torch.int64) & 0xFFFFFFFF) if words else z

    def policy_state(self) -> Dict[str, np.ndarray]:
        """The policy's own state for a checkpoint (npb_policy_get_state): ``t``, its draw counter; with a core, and only then, also
        ``hidden`` float32 [n, H], ``seen`` and ``primed`` int32 [n] (npb_policy_core_get_state)"""
        pol = self._on("_pol")
        t = ctypes.c_uint64()
        _lib.check(self.L.npb_policy_get_state(self._h, ctypes.byref(t)), self._h)
        out = {"t": np.uint64(t.value)}
        if pol["spec"]["core"] is not None:
            out.update(self._get_state("_pol", self.L.npb_policy_core_get_state))
        return out

    def load_policy_state(self, state) -> None:
        """put back what ``policy_state()`` returned (npb_policy_set_state): the noise resumes at that draw"""
        pol = self._on("_pol")
        _lib.check(self.L.npb_policy_set_state(self._h, int(state["t"])), self._h)
        if pol["spec"]["core"] is not None:
            self._load_state("_pol", self.L.npb_policy_core_set_state, state)

    def policy_spec(self) -> dict:
        """the request as data: what ``nuclear_sim_amd.policy.Policy`` takes (``core``, the cell's width, and ``gates`` are None without
        a core; with one, ``nuclear_sim_amd.recurrent.Policy`` takes them)"""
        return self._on("_pol")["spec"]

    def collect(self, steps: int) -> dict:
        """``steps`` steps in one call (npb_collect): with a policy and a rollout set nothing of a step comes from Python, so a whole
        rollout runs without it -- every buffer as ``steps`` calls of ``step()`` leave it.  Refused by name where a step input comes from
        the caller: an external heat source, host-side noise or a host-side power profile (episode streams drive both on the device), or a
        rollout without room.  Returns ``rollout()``."""
        self._on("_pol")
        self._on("_roll")
        if self.heat_source == "external":
            raise _lib.NpbError("collect() under heat_source='external': the heat source's power comes from the caller every step")
        if self._streams is None and (self._noise is not None or self.params.hs_noise_enabled):
            raise _lib.NpbError("collect() with host-side noise: the heat-source noise comes from the caller every step (enable_episode_streams drives it on the device)")
        if self._streams is None and self._profile is not None:
            raise _lib.NpbError("collect() with a host-side power profile: its rows come from the caller every step (enable_episode_streams drives it on the device)")
        self._keep = []
        self.features()
        _lib.check(self.L.npb_collect(self._h, int(steps), self._p(self._obs), self._p(self._reward), self._p(self._done), self._p(self._flags),
                                      self._p(self._info_buf), self._stream()), self._h)
        if self._feat is not None:
            self._feat["unprimed"] = False
        return self.rollout()

    def _order_buffers(self):
        """the buffers the perform_*_maintenance methods keep for their order columns, with the ``success`` column they all return"""
        if getattr(self, "_orders", None) is None:
            self._orders = {}
            with torch.cuda.device(self.device):
                self._orders["success"] = torch.zeros(self.n, dtype=torch.uint8, device=self.device)

    def _order_column(self, key, value, dtype, to_number):
        """one column of perform_maintenance's order: a device tensor of the right type is passed as it is, anything else lands in a
        buffer the env keeps (a scalar by fill_, an array by one copy); ``to_number`` maps a name to its index"""
        if isinstance(value, torch.Tensor) and value.device == self.device and value.dtype == dtype and value.shape == (self.n,) and value.is_contiguous():
            return value
        buf = self._orders.get(key)
        if buf is None:
            with torch.cuda.device(self.device):
                buf = self._orders[key] = torch.empty(self.n, dtype=dtype, device=self.device)
        if isinstance(value, torch.Tensor):
            buf.copy_(value.expand(self.n), non_blocking=True)
        else:
            a = np.asarray(to_number(value) if isinstance(value, str) or value is None else value)
            if a.size == 1:
                buf.fill_(a.reshape(()).item())
            else:
                buf.copy_(torch.as_tensor(np.array(np.broadcast_to(a, (self.n,)))))
        return buf

    def _masked_order(self, a, mask):
        """the action column with -1 (nothing ordered) where ``mask`` is 0; None = the column as it is"""
        if mask is None:
            return a
        m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.array(np.broadcast_to(np.asarray(mask), (self.n,))))
        none = self._orders.get("none")
        if none is None:
            with torch.cuda.device(self.device):
                none = self._orders["none"] = torch.empty(self.n, dtype=torch.bool, device=self.device)
                self._orders["masked"] = torch.empty(self.n, dtype=torch.int32, device=self.device)
        if m.device != self.device:
            m = m.to(self.device, non_blocking=True)
        torch.eq(m.expand(self.n), 0, out=none)
        masked = self._orders["masked"]
        masked.copy_(a)         # the caller's own column is left as it is
        return masked.masked_fill_(none, _lib.MAINT_ACTION_NONE)

    def perform_maintenance(self, action, pump, mask=None, bearing=None, target_level=None) -> torch.Tensor:
        """Operator-ordered maintenance between two steps (npb_perform_maintenance): what the reference's
        ``pump.perform_maintenance(action, **kwargs)`` (feedwater/pump_system.py:750, the lubrication system's dispatcher
        pump_lubrication.py:625-674) does to the ordered pump of every ordered plant, at once, on the device.

        ``action``: a name of ``_lib.MAINT_ACTIONS``, its index, or an int32 column (``-1`` = nothing for that plant); an unknown name
        raises ValueError before any device work.  ``pump``: 0..3, ``"FWP-1"``..``"FWP-4"``, or an int32 column.  ``mask`` (column,
        nonzero = ordered) turns the order into ``-1`` where it is 0.  ``bearing``: the ``component_id`` of a bearing replacement --
        None / ``"all"`` / ``"motor_bearings"`` / ``"pump_bearings"`` / ``"thrust_bearing"`` / NPB_BEARING_* / a column.
        ``target_level``: the oil top-off's target, default 95.0 as the reference's argument (not ``params.maint_top_off_target``,
        which the automatic maintenance uses).  Returns the ``success`` column (uint8; one of the env's own buffers, like step()'s
        outputs): 1 where the reference's result dict has ``'success': True``.  An action without a handler, a pump or bearing that does
        not exist: success 0, state untouched.  No host synchronisation, and with scalars or device columns no allocation after the first call
        (a host array is copied to the device, as step()'s inputs are).

        Only the ordered pump's state changes: no work order is created, ``info["maintenance_event_count"]`` and the ``maint.*`` /
        ``mpump.*`` columns do not move (the reference's direct call bypasses AutoMaintenanceSystem too); with the maintenance log
        on, each successful order is one ``operator_maintenance`` record.  Steam generators and condenser:
        ``perform_component_maintenance``; the turbine: ``perform_turbine_maintenance``.  Not covered: operator-created work orders,
        and -- with ``enable_diagnostics`` -- the
        per-pump ``maintenance_occurred`` / ``oil_top_off_occurred`` / ``maintenance_action`` diagnostics rows, which an operator
        action leaves alone."""
        if isinstance(action, str):
            action = _lib.maint_action_index(action)       # ValueError for an unknown name, before anything else
        if isinstance(pump, str):
            if pump not in _lib.PUMP_IDS:
                raise ValueError("unknown feedwater pump %r: one of %r" % (pump, _lib.PUMP_IDS))
            pump = _lib.PUMP_IDS.index(pump)
        if isinstance(bearing, str) and bearing not in _lib.MAINT_BEARINGS:
            raise ValueError("unknown bearing %r: one of %r" % (bearing, [k for k in _lib.MAINT_BEARINGS if k]))
        if not hasattr(self.L, "npb_perform_maintenance"):
            raise _lib.NpbError("libnpb.so has no npb_perform_maintenance (older than ABI 147): rebuild")
        self._order_buffers()
        a = self._masked_order(self._order_column("action", action, torch.int32, _lib.maint_action_index), mask)
        k = self._order_column("pump", pump, torch.int32, _lib.PUMP_IDS.index)
        b = None if bearing is None else self._order_column("bearing", bearing, torch.int32, _lib.MAINT_BEARINGS.__getitem__)
        lvl = None if target_level is None else self._order_column("target_level", target_level, torch.float64, float)
        ok = self._orders["success"]
        _lib.check(self.L.npb_perform_maintenance(self._h, self._p(a), self._p(k), self._p(b), self._p(lvl), self._p(ok), self._stream()), self._h)
        return ok

    def perform_component_maintenance(self, component, action, unit=None, mask=None, cleaning_type=None, tubes_to_plug=None) -> torch.Tensor:
        """Operator-ordered maintenance of a steam generator, the steam-generator system, the condenser or a steam-jet ejector between
        two steps (npb_perform_component_maintenance): what the reference's ``perform_maintenance(action, **kwargs)`` of that object
        (steam_generator/steam_generator.py:1092, steam_generator/enhanced_physics.py:1062, condenser/physics.py:1188,
        condenser/vacuum_pump.py:338) does to every ordered plant, at once, on the device.

        ``component``: ``"steam_generator"``, ``"steam_generator_system"``, ``"condenser"`` or ``"ejector"``.  ``action``: a maintenance
        type of that component in ``_lib.COMPONENT_ACTIONS``, its catalog index, or an int32 column of catalog indices (``-1`` = nothing
        for that plant; the index names the component, so a column may mix kinds); an unknown name raises ValueError before any device
        work, and so does, with its own message, a handler that is not offered (``_lib.COMPONENT_ACTIONS_NOT_OFFERED``).  ``unit``: the
        generator 0..2 or the ejector 0..1 / ``"SJE-001"`` / ``"SJE-002"``, or an int32 column; None = 0; ignored by system and condenser
        actions.  ``mask`` as in ``perform_maintenance``.  ``cleaning_type``: None (the handler's default argument, "chemical"),
        ``"chemical"`` / ``"mechanical"`` / ``"hydroblast"`` / ``"replacement"``, any other string (the handlers' "anything else"), an
        NPB_CLEANING_* index or a column.  ``tubes_to_plug``: the kwarg of condenser_tube_plugging, carried by the ABI for the day that
        handler can be offered; no offered handler reads it.  Returns the ``success`` column (uint8, the env's own buffer): 1 where the
        reference's result says success.  No host synchronisation.

        Only the sections the action touches change, on the ordering plants only.  No work order, counter, ``maint.*`` / ``mpump.*``
        column moves; with the maintenance log on, each successful order is one ``operator_component_maintenance`` record.  The
        state-log columns that show attributes the state does not carry (a generator's cleaning cycles and years since cleaning, the
        chemistry's time since treatment) do not follow an operator action.  Not covered: work orders for these components.  The
        turbine: ``perform_turbine_maintenance``."""
        if isinstance(action, str) or component not in _lib.COMPONENT_KINDS:
            action = _lib.component_action_index(component, action)       # ValueError for an unknown kind or name, before anything else
        if isinstance(unit, str):
            if component != "ejector" or unit not in _lib.EJECTOR_IDS:
                raise ValueError("unknown unit %r of a %s" % (unit, component))
            unit = _lib.EJECTOR_IDS.index(unit)
        if not hasattr(self.L, "npb_perform_component_maintenance"):
            raise _lib.NpbError("libnpb.so has no npb_perform_component_maintenance (older than ABI 148): rebuild")
        self._order_buffers()
        a = self._masked_order(self._order_column("component_action", action, torch.int32, int), mask)
        k = None if unit is None else self._order_column("unit", unit, torch.int32, int)
        if isinstance(cleaning_type, str):
            cleaning_type = _lib.cleaning_type_index(cleaning_type)
        c = None if cleaning_type is None else self._order_column("cleaning_type", cleaning_type, torch.int32, int)
        amount = None if tubes_to_plug is None else self._order_column("tubes_to_plug", tubes_to_plug, torch.float64, float)
        ok = self._orders["success"]
        _lib.check(self.L.npb_perform_component_maintenance(self._h, self._p(a), self._p(k), self._p(c), self._p(amount), self._p(ok), self._stream()), self._h)
        return ok

    def perform_turbine_maintenance(self, component, action, unit=None, mask=None) -> torch.Tensor:
        """Operator-ordered maintenance of the turbine, one of its bearings, its bearing-lubrication system or one of its stages between
        two steps (npb_perform_turbine_maintenance): what the reference's ``perform_maintenance(action)`` of that object
        (turbine/enhanced_physics.py:1055, turbine/rotor_dynamics.py:381, turbine/turbine_bearing_lubrication.py:481,
        turbine/stage_system.py:341) does to every ordered plant, at once, on the device.

        ``component``: ``"turbine"``, ``"bearing"``, ``"lubrication"`` or ``"stage"``.  ``action``: a maintenance type of that component
        in ``_lib.TURBINE_ACTIONS``, its catalog index, or an int32 column of catalog indices (``-1`` = nothing for that plant; the index
        names the component, so a column may mix kinds); an unknown name raises ValueError before any device work, and so does, with its
        own message, a handler that is not offered because the carried state cannot hold what it does
        (``_lib.TURBINE_ACTIONS_NOT_OFFERED``: a stage's ``"cleaning"``).  ``unit``: the bearing 0..3 / ``"TB-001"``..``"TB-004"`` or the
        stage 0..13 / ``"HP-1"``..``"LP-6"``, or an int32 column; None = 0; ignored by actions on the turbine and the lubrication system.
        ``mask`` as in ``perform_maintenance``.  Returns the ``success`` column (uint8, the env's own buffer): 1 where the reference's
        result says success; ``thrust_bearing_adjustment`` succeeds on the thrust bearing (2, ``"TB-003"``) only; in the modes that do not
        step the turbine (``primary``, ``primary_sg``) every order gives 0.  No host synchronisation.

        Only ``turb.*`` members change, or the ordered stage's ``tstg.stage_deposit_thickness`` / ``stage_blade_wear_factor`` /
        ``stage_efficiency_degradation``, on the ordering plants only.  No work order, counter, ``maint.*`` / ``mpump.*`` column moves;
        with the maintenance log on, each successful order is one ``operator_turbine_maintenance`` record.  With
        ``enable_diagnostics`` the accumulator rows (the bearings' clearance increase, the stage system's efficiency) do not follow an
        operator action, nor do the state-log columns that show attributes the state does not carry.  Not covered: work orders and
        automatic maintenance for the turbine, and the single-plant facade (``NuclearPlantSimulator``'s turbine has no
        ``perform_maintenance``: out of scope here)."""
        from . import maintlog
        if isinstance(action, str) or component not in _lib.TURBINE_KINDS:
            action = _lib.turbine_action_index(component, action)       # ValueError for an unknown kind or name, before anything else
        if isinstance(unit, str):
            ids = {"bearing": maintlog.TURBINE_BEARING_IDS, "stage": maintlog.TURBINE_STAGE_IDS}.get(component, ())
            if unit not in ids:
                raise ValueError("unknown unit %r of a turbine %s" % (unit, component))
            unit = ids.index(unit)
        if not hasattr(self.L, "npb_perform_turbine_maintenance"):
            raise _lib.NpbError("libnpb.so has no npb_perform_turbine_maintenance (older than ABI 149): rebuild")
        self._order_buffers()
        a = self._masked_order(self._order_column("turbine_action", action, torch.int32, int), mask)
        k = None if unit is None else self._order_column("unit", unit, torch.int32, int)
        ok = self._orders["success"]
        _lib.check(self.L.npb_perform_turbine_maintenance(self._h, self._p(a), self._p(k), self._p(ok), self._stream()), self._h)
        return ok

    def snapshot(self) -> None:
        """Record every plant's current state as its episode start (npb_snapshot: one device-to-device copy of the arena).  Call it
        after ``set_fields`` has put the initial conditions in; ``restore`` and the autoreset go back to it."""
        _lib.check(self.L.npb_snapshot(self._h, self._stream()), self._h)

    def restore(self, mask=None) -> torch.Tensor:
        """The plants of ``mask`` (None = all) back to the state ``snapshot()`` recorded -- unlike ``reset()``, with their own initial
        conditions -- and their episode counters to zero.  Returns the observation, as ``reset()`` does."""
        m = self._col(mask, torch.uint8)
        self._reset_carried_diagnostics(m)
        _lib.check(self.L.npb_restore(self._h, self._p(m), self._stream()), self._h)
        self._after_restart(m)
        return self.get_observation()

    def set_start_bank(self, bank_env: Optional["BatchedPlantEnv"], slots=None, advance: Optional[int] = None) -> None:
        """Copy the states of ``bank_env``'s M plants (same storage type and device; ``self`` allowed) into a start bank
        (npb_set_start_bank: one device-to-device copy); the autoreset and ``restore_from_bank`` then restore plant p from entry
        ``next_start_slots[p] mod M`` and advance that slot by ``advance``.  ``slots`` defaults to ``arange(n) % M`` and
        ``advance`` to n, so plant p walks through entries p, p + n, p + 2n, ... mod M; with ``advance = 0`` the caller picks
        every restart by writing ``next_start_slots``.  ``bank_env = None`` frees the bank."""
        if bank_env is None:
            _lib.check(self.L.npb_set_start_bank(self._h, None, self._stream()), self._h)
            self._bank = None
            return
        adv = self.n if advance is None else int(advance)
        if adv < 0:
            raise ValueError("advance must be >= 0")
        _lib.check(self.L.npb_set_start_bank(self._h, bank_env._h, self._stream()), self._h)
        M = bank_env.n
        with torch.cuda.device(self.device):
            if self._bank is None:
                self.next_start_slots = torch.zeros(self.n, dtype=torch.int32, device=self.device)
                self.episode_start = torch.full((self.n,), -1, dtype=torch.int32, device=self.device)
                self._episode_start_out = torch.full((self.n,), -1, dtype=torch.int32, device=self.device)
            if slots is None:
                self.next_start_slots.copy_(torch.arange(self.n, device=self.device) % M)
            else:
                self.next_start_slots.copy_(self._col(slots, torch.int32))
        _lib.check(self.L.npb_set_start_slots(self._h, self._p(self.next_start_slots), self._p(self.episode_start), adv), self._h)
        _lib.check(self.L.npb_set_episode_start_buffer(self._h, self._p(self._episode_start_out)), self._h)
        self._bank = {"entries": M, "advance": adv}

    def restore_from_bank(self, mask=None) -> torch.Tensor:
        """The plants of ``mask`` (None = all) from their bank entries (``set_start_bank``; npb_restore_bank), their slots
        advanced and their episode counters to zero.  Returns the observation, as ``restore()`` does."""
        m = self._col(mask, torch.uint8)
        self._reset_carried_diagnostics(m)
        _lib.check(self.L.npb_restore_bank(self._h, self._p(m), self._stream()), self._h)
        self._after_restart(m)
        return self.get_observation()

    def _enable_autoreset(self, max_episode_steps: Optional[int]) -> None:
        """npb_set_autoreset on the snapshot taken, and the four info columns the episode kernel writes"""
        with torch.cuda.device(self.device):
            self._episode = {"truncated": torch.zeros(self.n, dtype=torch.uint8, device=self.device),
                             "final_observation": torch.zeros((self.n, 22), dtype=torch.float64, device=self.device),
                             "episode_length": torch.zeros(self.n, dtype=torch.int32, device=self.device),
                             "episode_return": torch.zeros(self.n, dtype=torch.float64, device=self.device)}
            if hasattr(self.L, "npb_set_episode_index_buffer"):
                self._episode["episode_index"] = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        _lib.check(self.L.npb_set_autoreset(self._h, 1, int(max_episode_steps or 0)), self._h)
        self._max_episode_steps = int(max_episode_steps or 0)
        e = self._episode
        _lib.check(self.L.npb_set_episode_buffers(self._h, self._p(e["episode_length"]), self._p(e["episode_return"]), self._p(e["truncated"]),
                                                  self._p(e["final_observation"])), self._h)
        if "episode_index" in e:
            _lib.check(self.L.npb_set_episode_index_buffer(self._h, self._p(e["episode_index"])), self._h)

    def enable_episode_streams(self, block: int = 64, bank_noise_seeds=None, bank_profile_seeds=None) -> None:
        """Switch episode streams on (the class docstring; npb_set_episode_streams): the handle draws both streams ``block`` rows at a
        time and restarts a plant's with its episode.  ``bank_noise_seeds`` / ``bank_profile_seeds``: one seed per entry of the start
        bank, for the restarts that take that entry; without a table such a restart uses the plant's own seed again.  Switching on is
        itself a restart of every plant from its own seeds.  Needs autoreset and device generators."""
        if not hasattr(self.L, "npb_set_episode_streams"):
            raise _lib.NpbError("libnpb.so has no npb_set_episode_streams: rebuild")
        if self._noise is not None and not isinstance(self._noise, DeviceHeatSourceNoise):
            raise ValueError("episode_streams needs noise_generator='device': the host generator's pre-drawn stream cannot restart per plant on the device")
        with torch.cuda.device(self.device):
            out = torch.zeros((3, self.n), dtype=torch.float64, device=self.device)
        desc, keep = _lib.episode_streams_desc(block, bank_noise_seeds, bank_profile_seeds, [int(out[k].data_ptr()) for k in range(3)])
        _lib.check(self.L.npb_set_episode_streams(self._h, ctypes.byref(desc), self._stream()), self._h)
        del keep      # (the call has copied the tables)
        self._streams = {"noise": out[0], "setpoint": out[1], "target": out[2]}

    def disable_episode_streams(self) -> None:
        """Episode streams off again: every plant's streams begin anew from its own seeds, and run on across restarts as before."""
        _lib.check(self.L.npb_set_episode_streams(self._h, None, self._stream()), self._h)
        self._streams = None
        for stream in (self._noise, self._profile):      # nothing of a block handed out before the mode is left
            if stream is not None:
                stream._buf, stream._pos = None, stream._block

    @property
    def stream_rows(self) -> Optional[Dict[str, torch.Tensor]]:
        """episode streams: the rows the last ``step()`` took from the handle's streams, [n] float64 each (the env's own buffers, written
        again by the next step; a stream the caller overrode on that step keeps its earlier row); None while the mode is off"""
        return self._streams

    def profile_positions(self):
        """episode streams: ``(position, rows_made)`` of every plant's power profile, int32 [n] numpy arrays -- the row of its current
        profile the next row made for it is, and the rows made for it since its restart, drawn ahead included (npb_profile_get_positions)"""
        position, rows_made = np.empty(self.n, dtype=np.int32), np.empty(self.n, dtype=np.int32)
        _lib.check(self.L.npb_profile_get_positions(self._h, position.ctypes.data_as(ctypes.c_void_p), rows_made.ctypes.data_as(ctypes.c_void_p),
                                                    self._stream()), self._h)
        return position, rows_made

    def _refuse_in_episode_streams(self, who: str) -> None:
        if self._streams is not None:
            raise _lib.NpbError("%s: episode streams are on, and the handle owns the streams' consumption (step() takes its rows; "
                                "disable_episode_streams() first)" % who)

    def log_sources(self) -> Dict[str, torch.Tensor]:
        """The buffers beside the arena that a state log with a watch list samples (nuclear_sim_amd/statelog.py, ``sample_request``): the
        step's info block, its ``done`` column, the diagnostics buffer while the diagnostics are on and the episode columns of an env
        with autoreset.  The env owns them; the log reads them through its sampler (npb_sampler_create)."""
        out = {"info": self._info_buf, "done": self._done}
        if self._diag_buf is not None:
            out["diagnostics"] = self._diag_buf
        if self._episode is not None:
            out.update({k: self._episode[k] for k in ("truncated", "episode_index", "episode_length") if k in self._episode})
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.L.npb_destroy(self._h)
            self._h = ctypes.c_void_p()
        self._erec = None      # the episode records' buffers go with the handle
        self._cstats = None
        self._ewin = None      # (the handle has freed the ring; the record columns go with it)
        self._task = None
        self._feat = None
        self._ctl = None
        self._ord = None
        self._roll = None
        self._norm = None
        self._pol = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _col(self, x, dtype):
        """None | scalar | array | tensor -> device tensor of shape [n] (kept alive until the next step)."""
        if x is None:
            return None
        if isinstance(x, torch.Tensor):
            t = x.to(device=self.device, dtype=dtype).expand(self.n).contiguous()
        else:
            a = np.asarray(x)
            if a.size == 1:      # the same value for every plant: filled on the device, nothing to copy
                t = torch.full((self.n,), a.reshape(()).item(), dtype=dtype, device=self.device)
            else:
                t = torch.as_tensor(np.array(np.broadcast_to(a, (self.n,))), dtype=dtype).to(self.device)
        self._keep.append(t)
        return t

    @staticmethod
    def _p(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    # ------------------------------------------------------------------ state columns
    def get_field(self, name: str, instance: int = 0, k: int = 0) -> torch.Tensor:
        return self._get_slot(*SCHEMA.slot(name, instance, k))

    def set_field(self, name: str, value, instance: int = 0, k: int = 0) -> None:
        self._set_slot(*SCHEMA.slot(name, instance, k), value)

    def _get_slot(self, kind: str, slot: int) -> torch.Tensor:
        t = torch.empty(self.n, dtype=torch.float64 if kind == "f64" else torch.int32, device=self.device)
        _lib.check(self.L.npb_get_field(self._h, 0 if kind == "f64" else 1, slot, self._p(t), 1, self._stream()), self._h)
        return t

    def _set_slot(self, kind: str, slot: int, value) -> None:
        t = self._col(value, torch.float64 if kind == "f64" else torch.int32)
        _lib.check(self.L.npb_set_field(self._h, 0 if kind == "f64" else 1, slot, self._p(t), 1, self._stream()), self._h)

    def set_fields(self, fields: dict) -> None:
        for key, v in fields.items():
            if isinstance(key, tuple):
                self.set_field(key[0], v, *key[1:])
            else:
                self.set_field(key, v)

    def state_arrays(self):
        """(f64[total_f64, n], i32[total_i32, n]) copies of the whole arena (testing / checkpointing).  A full checkpoint is up to three
        things: these arrays, ``component_maintenance_state()`` where ``component_maintenance`` is on, and ``diagnostics_state()`` on an
        env with ``diagnostics=True`` (the rows the diagnostics build carries from step to step live in its buffer, not in the arena)."""
        f = torch.empty((SCHEMA.total_f64, self.n), dtype=torch.float64, device=self.device)
        i = torch.empty((SCHEMA.total_i32, self.n), dtype=torch.int32, device=self.device)
        for s in range(SCHEMA.total_f64):
            _lib.check(self.L.npb_get_field(self._h, 0, s, ctypes.c_void_p(f[s].data_ptr()), 1, self._stream()), self._h)
        for s in range(SCHEMA.total_i32):
            _lib.check(self.L.npb_get_field(self._h, 1, s, ctypes.c_void_p(i[s].data_ptr()), 1, self._stream()), self._h)
        return f, i

    def component_maintenance_state(self) -> torch.Tensor:
        """[_lib.CMAINT_SIDE_DOUBLES, n] copy of the side state of the automatic maintenance of steam generators and condenser
        (npb_get_component_maintenance_state; rows: member of _lib.CMAINT_STATE_MEMBERS x (component of _lib.CMAINT_COMPONENTS x row),
        include/npb_maint.h).  It is plant state that lives outside the arena: a checkpoint saves it beside ``state_arrays()``."""
        t = torch.empty((_lib.CMAINT_SIDE_DOUBLES, self.n), dtype=torch.float64, device=self.device)
        assert int(self.L.npb_component_maintenance_state_bytes(self._h)) == t.numel() * 8
        _lib.check(self.L.npb_get_component_maintenance_state(self._h, self._p(t), self._stream()), self._h)
        return t

    def load_component_maintenance_state(self, state) -> None:
        """the inverse of ``component_maintenance_state`` (npb_set_component_maintenance_state)"""
        t = torch.as_tensor(state, dtype=torch.float64).to(self.device).contiguous()
        if t.shape != (_lib.CMAINT_SIDE_DOUBLES, self.n):
            raise ValueError("component maintenance state must be [%d, %d]" % (_lib.CMAINT_SIDE_DOUBLES, self.n))
        _lib.check(self.L.npb_set_component_maintenance_state(self._h, self._p(t), self._stream()), self._h)

    def load_state_arrays(self, f64, i32) -> None:
        """the inverse of ``state_arrays``; a full checkpoint also loads ``load_component_maintenance_state`` where that feature is on
        and ``load_diagnostics_state`` on an env with ``diagnostics=True`` (see ``state_arrays``)"""
        f = torch.as_tensor(f64, dtype=torch.float64).to(self.device).contiguous()
        i = torch.as_tensor(i32, dtype=torch.int32).to(self.device).contiguous()
        for s in range(SCHEMA.total_f64):
            _lib.check(self.L.npb_set_field(self._h, 0, s, ctypes.c_void_p(f[s].data_ptr()), 1, self._stream()), self._h)
        for s in range(SCHEMA.total_i32):
            _lib.check(self.L.npb_set_field(self._h, 1, s, ctypes.c_void_p(i[s].data_ptr()), 1, self._stream()), self._h)
        torch.cuda.synchronize(self.device)

    @staticmethod
    def state_bytes_per_plant() -> int:
        return int(_lib.load().npb_state_bytes())

    @staticmethod
    def step_bytes_per_plant() -> int:
        return int(_lib.load().npb_step_bytes_per_plant())

    def handle_step_bytes_per_plant(self) -> int:
        """Algorithmic bytes of one plant-step for this handle's storage type."""
        return int(self.L.npb_handle_step_bytes_per_plant(self._h))

    # ------------------------------------------------------------------ reference API
    def reset(self, mask=None, reference: bool = False, start_at_steady_state: bool = True) -> torch.Tensor:
        """``reference=False``: back to the construction-time state, i.e. a freshly constructed simulator (the
        episode start of the data-gen runner, which never calls reset()).  ``reference=True``:
        NuclearPlantSimulator.reset(start_at_steady_state) with the reference's own semantics (sim.py:546-581): part of
        the state goes back to literals, part keeps its history, and with ``start_at_steady_state`` the secondary side
        is force-set to the reference's "steady state" (include/npb.h, npb_reset_reference).  Initial conditions set
        through ``set_fields`` are the caller's to re-apply.  Returns the observation, as the reference does."""
        m = self._col(mask, torch.uint8)
        self._reset_carried_diagnostics(m)
        if reference:
            _lib.check(self.L.npb_reset_reference(self._h, self._p(m), int(bool(start_at_steady_state)), self._stream()), self._h)
        else:
            _lib.check(self.L.npb_reset(self._h, self._p(m), self._stream()), self._h)
            # a freshly constructed simulator has a freshly seeded heat-source generator (the reference's own reset() keeps
            # drawing from the old one: constant_heat_source.py:185-194 does not touch the RNG).  Plants that share a seed
            # share one pre-drawn stream here, so only a reset of the whole batch can restart it.
            # With episode streams the handle has restarted the streams of exactly the plants it reset, on the device.
            if mask is None and self._noise is not None and self._noise_seeds is not None and self._streams is None:
                self._noise = self._make_noise(self._noise_seeds)
            if mask is None and self._profile is not None and self._streams is None:      # and a freshly started runner a freshly drawn profile
                self._profile = PowerProfile(self, **self._profile_args)
        self._after_restart(m)
        return self.get_observation()

    def ramp_setpoints(self, targets: torch.Tensor) -> torch.Tensor:
        """The runner's ``_set_target_power`` for a block of targets ([k, n] float64 on the device, or one [n] row): the setpoints
        the heat source is to be given, each at most 0.02 % from the one before (npb_profile_ramp).  The previous setpoint is carried
        in the handle from call to call; the very first call starts on its first target.  ``forget_ramp()`` starts afresh."""
        t = targets.reshape(-1, self.n)
        if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
            t = t.to(device=self.device, dtype=torch.float64).contiguous()
        out = torch.empty_like(t)
        _lib.check(self.L.npb_profile_ramp(self._h, t.shape[0], ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(out.data_ptr()), self._stream()), self._h)
        return out.reshape(targets.shape)

    def forget_ramp(self) -> None:
        """drop the setpoints ``ramp_setpoints`` carries: its next call starts on its first target"""
        _lib.check(self.L.npb_profile_ramp(self._h, 0, None, None, self._stream()), self._h)

    def get_observation(self) -> torch.Tensor:
        _lib.check(self.L.npb_observe(self._h, self._p(self._obs), self._stream()), self._h)
        return self._obs

    def secondary_result(self) -> Dict[str, torch.Tensor]:
        """info["secondary_system"] of the reference for every plant, as columns, for the step just taken (one gather launch)"""
        if getattr(self, "_sec_plan", None) is None:
            ks = [SCHEMA.slot(name) for name in SECONDARY_RESULT_MEMBERS]
            self._sec_plan = ((ctypes.c_int * len(ks))(*[0 if kd == "f64" else 1 for kd, _ in ks]), (ctypes.c_int * len(ks))(*[sl for _, sl in ks]))
            self._sec_buf = torch.empty((len(ks), self.n), dtype=torch.float64, device=self.device)
        _lib.check(self.L.npb_gather_fields(self._h, len(SECONDARY_RESULT_MEMBERS), self._sec_plan[0], self._sec_plan[1],
                                            ctypes.c_void_p(self._sec_buf.data_ptr()), self._stream()), self._h)
        members = {name: self._sec_buf[j] for j, name in enumerate(SECONDARY_RESULT_MEMBERS)}
        info = {name: self._info[:, j] for j, name in enumerate(INFO_COLUMNS)}
        return secondary_result(info, members)

    def step(self, action=None, magnitude=None, power_setpoint=None, cooling_water_temp=None, noise_z=None,
             thermal_power_mw=None, power_percent=None, controls=None):
        self._keep = []
        ctl = self._ctl
        if self._pol is not None:      # the policy reads the features in front of the step and is the one writer of the controls' input
            if controls is not None:
                raise _lib.NpbError("step(controls=...) while a policy is set: the policy writes the controls (set_policy(None) first)")
            self.features()
        if self._roll is not None:      # the rollout records the features in front of the step: every plant has a frame by then
            self.features()
        if controls is not None:      # the policy's output for this step (set_controls): into the bound tensor unless it is that tensor
            if ctl is None:
                raise _lib.NpbError("step(controls=...) without controls: set_controls() first")
            if not (isinstance(controls, torch.Tensor) and controls.data_ptr() == ctl["in"].data_ptr() and controls.dtype == ctl["in"].dtype):
                ctl["in"].copy_(torch.as_tensor(controls).to(device=self.device).reshape(ctl["in"].shape))
        if self.heat_source == "external":
            # the plugin's heat_result['thermal_power_mw'] / ['power_percent'] for this step travel in the noise_z / power_setpoint
            # columns of the C ABI (include/npb_params.h, NPB_HEAT_EXTERNAL); power_percent None = thermal power / rated x 100
            if thermal_power_mw is None:
                if noise_z is None:
                    raise ValueError("heat_source='external': step() needs the heat source's thermal_power_mw for this step")
                thermal_power_mw, power_percent = noise_z, power_setpoint       # (a caller that speaks the C ABI's column names)
            noise_z, power_setpoint = thermal_power_mw, power_percent
        elif thermal_power_mw is not None or power_percent is not None:
            raise ValueError("thermal_power_mw / power_percent are the inputs of heat_source='external'")
        a = self._col(None if action is None else action, torch.int32)
        m = self._col(magnitude, torch.float64)
        target_power = None
        if power_setpoint is None and self._profile is not None:
            if self._streams is not None:      # episode streams: no column; the handle takes its own row and reports it
                target_power = self._streams["target"]
            else:
                power_setpoint, target_power = self._profile.next()
        sp = self._col(power_setpoint, torch.float64)
        cw = self._col(cooling_water_temp, torch.float64)
        if noise_z is None and self._noise is None and self.params.hs_noise_enabled:
            # ConstantHeatSource(noise_enabled=True, noise_seed=None) draws from an unseeded generator
            # (constant_heat_source.py:58-62): one fresh, unseeded stream per plant
            self._noise = self._make_noise(np.random.SeedSequence().generate_state(self.n, dtype=np.uint32))
        if noise_z is None and self._noise is not None and self._streams is None:
            noise_z = self._noise.next()
        z = self._col(noise_z, torch.float64)
        _lib.check(self.L.npb_step(self._h, self._p(a), self._p(m), self._p(sp), self._p(z), self._p(cw),
                                   self._p(self._obs), self._p(self._reward), self._p(self._done), self._p(self._flags),
                                   self._p(self._info_buf), self._stream()), self._h)
        info = {name: self._info[:, j] for j, name in enumerate(INFO_COLUMNS)}
        if self._with_rho:
            info["reactivity_components"] = {name: self._rho[:, j] for j, name in enumerate(_lib.REACTIVITY_COMPONENTS)}
        info["trip_flags"] = self._flags
        info["scram_activated"] = self._done
        task = self._task
        if task is not None:      # the caller's reward and termination rule, formed behind the step (set_task)
            info["reference_reward"] = self._reward
            info["task_cause"] = task["cause"]
            if task["terms"] is not None:
                info["task_terms"] = task["terms"]
        if target_power is not None:   # the power profile's row before the ramp: the runner's target_power for this step
            info["target_power"] = target_power
        if self.params.maint_enabled:  # bit-exact counterpart of AutoMaintenanceSystem.maintenance_actions_performed
            # a column the step keeps current (npb_set_maintenance_count_buffer): no gather launch per step
            info["maintenance_event_count"] = self._event_counts if self._event_counts is not None else self.get_field("maint.maintenance_actions_performed")
        if self._episode is not None:     # autoreset: written by the episode kernel behind the step (npb_set_autoreset)
            info.update(self._episode)
            if self._bank is not None:    # the episode kernel's, restoring from the bank: the bank entry this transition's episode started from
                info["episode_start"] = self._episode_start_out
        if ctl is not None:      # the action every plant is under after this step's decode: [n_axes, n] (set_controls)
            info["controls"] = ctl["held"]
        if self._ord is not None:      # which rule fired on which plant on this step: [n_orders, n] (set_control_orders)
            info["orders"] = self._ord["fired"]
        obs = self._obs
        feat = self._feat
        if feat is not None:      # the caller's policy inputs, kept behind the step (set_features)
            feat["unprimed"] = False
            info["features"] = feat["out"]
            if self._episode is not None and feat["final"] is not None:
                info["final_features"] = feat["final"]
            if feat["as_observation"]:
                info["observation"] = obs
                obs = feat["out"]
        if self._norm is not None and self._norm["norm_reward"] is not None:      # the reward the learner sees (set_normalizer); the one returned stays raw
            info["norm_reward"] = self._norm["norm_reward"]
        if self._pol is not None:      # what the policy made of the features in front of this step (set_policy)
            info["value"], info["logp"] = self._pol["value"], self._pol["logp"]
        if task is not None:
            return obs, task["reward"], task["done"], info
        return obs, self._reward, self._done, info


def secondary_result(info: Dict[str, torch.Tensor], members: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The scalar keys of the reference's info["secondary_system"] (SecondaryReactorPhysics.update_system's result dict,
    secondary/__init__.py:922-1010) as columns, including its heat-flow and chemistry-flow tracker outputs
    (heat_flow_tracker.py:248-351, chemistry_flow_tracker.py:472-666; consumed at secondary/__init__.py:979-994).
    ``info`` = the step's fp64 info columns, ``members`` = the state members named in SECONDARY_RESULT_MEMBERS.
    The trackers are bookkeeping on top of quantities the step already has: the heat-flow state is closed-form in the SG
    heat transfer, the turbine power and the feedwater pump power (secondary/__init__.py:679-744); the chemistry-flow tracker
    looks its providers' states up under ChemicalSpecies names that none of them uses ("ph", "iron" ... vs
    "water_chemistry_ph" ...), so every lookup takes its default and its seven outputs are constants."""
    f = {}
    total_heat_transfer = info["sg_heat_transfer"]; turbine_gross = info["turbine_power"]; fw_power = info["feedwater_power"]
    electrical = info["electrical_power"]
    zero = torch.zeros_like(electrical); one = torch.ones_like(electrical)
    f["electrical_power_mw"] = members["sec.electrical_power_output"]
    f["thermal_efficiency"] = members["sec.thermal_efficiency"]
    f["heat_rate_kj_kwh"] = torch.where(electrical > 0, (total_heat_transfer / 1000.0) / (electrical * 1000.0) * 3600.0, zero)
    f["total_steam_flow"] = info["steam_flow"]; f["total_heat_transfer"] = total_heat_transfer; f["sg_total_heat_transfer"] = total_heat_transfer
    f["total_feedwater_flow"] = info["feedwater_flow"]; f["feedwater_total_flow"] = info["feedwater_flow"]
    f["sg_avg_pressure"] = info["steam_pressure"]
    # reported (not used by the turbine) as max(SG average, saturation temperature at the average pressure)
    # secondary/__init__.py:551-552 with _saturation_temperature :1455-1491
    pr = info["steam_pressure"] / 0.101325
    sat = 1.0 / (1.0 / (100.0 + 273.15) - (0.4615 / 2257.0) * torch.log(pr.clamp_min(1e-300))) - 273.15
    sat = torch.where(info["steam_pressure"] <= 0.001, torch.full_like(sat, 10.0), sat.clamp(10.0, 374.0))
    f["sg_avg_temperature"] = torch.maximum(members["sec.sg_avg_temperature"], sat); f["sg_avg_steam_quality"] = members["sec.sg_avg_quality"]
    mechanical = turbine_gross / 0.985
    f["turbine_mechanical_power"] = mechanical; f["turbine_electrical_power_gross"] = turbine_gross
    f["turbine_electrical_power_net"] = turbine_gross * 0.98
    f["turbine_steam_rate"] = torch.where(turbine_gross > 0, info["steam_flow"] / (turbine_gross * 1000) * 3600, zero)
    f["condenser_heat_rejection"] = members["cond.heat_rejection_rate"]; f["condenser_pressure"] = info["condenser_pressure"]
    f["condenser_vacuum_efficiency"] = members["cond.vacuum_system_efficiency"]
    f["total_system_heat_rejection"] = info["condenser_heat_rejection"]
    f["feedwater_total_power"] = fw_power
    mask = members["fw.running_mask"].to(torch.int64)
    f["feedwater_num_running_pumps"] = ((mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1)).to(torch.float64)
    f["feedwater_system_available"] = members["fw.system_availability"]
    # ---- HeatFlowTracker: component flows secondary/__init__.py:686-736, system state heat_flow_tracker.py:248-322
    sg_in = total_heat_transfer / 1e6; sg_out = total_heat_transfer * 0.98 / 1e6; sg_loss = total_heat_transfer * 0.02 / 1e6
    turb_loss = mechanical * 0.05
    fw_loss = fw_power * 0.1
    total_losses = (sg_loss + turb_loss + fw_loss)
    required_rejection = sg_in - mechanical - total_losses
    cond_loss = required_rejection * 0.01
    gen_out = mechanical * 0.985; gen_loss = mechanical - gen_out
    aux = gen_out * 0.02; net = gen_out - aux
    total_in = (sg_in + fw_power)
    total_out = (net + required_rejection + sg_loss + turb_loss + cond_loss + fw_loss + gen_loss + 0.0)
    err = total_in - total_out
    pct = torch.where(total_in > 0, (err / total_in) * 100.0, zero)
    f["heat_flow_energy_balance_error"] = err; f["heat_flow_energy_balance_percent"] = pct
    f["heat_flow_balance_ok"] = (pct.abs() < (0.01 * 100)).to(torch.float64)
    f["heat_flow_condenser_heat_rejection"] = required_rejection; f["heat_flow_net_electrical_output"] = net
    f["heat_flow_overall_efficiency"] = torch.where(total_in > 0, net / total_in, zero)
    # ---- ChemistryFlowTracker: every provider lookup falls through to its default (see the docstring)
    f["chemistry_flow_balance_error"] = zero; f["chemistry_flow_balance_ok"] = one; f["chemistry_flow_ph"] = one * 9.2
    f["chemistry_flow_iron_concentration"] = one * 0.1; f["chemistry_flow_tsp_fouling_rate"] = zero
    f["chemistry_flow_treatment_efficiency"] = one; f["chemistry_flow_stability"] = one * 0.5
    # ---- shared WaterChemistry and the pH controller
    f["water_chemistry_ph"] = members["chem.ph"]; f["water_chemistry_iron_concentration"] = one * 0.1
    f["water_chemistry_aggressiveness"] = members["chem.water_aggressiveness"]
    f["water_chemistry_treatment_efficiency"] = members["chem.treatment_efficiency"]
    f["ph_control_output"] = members["ph.controller_output"]; f["ph_control_ammonia_dose"] = members["ph.pending_ammonia_dose"]
    # ph_control_system.py:243: setpoint - measured, computed every step (previous_error only follows it while the controller is enabled)
    f["ph_control_error"] = 9.2 - members["ph.measured_ph"]
    f["load_demand"] = members["sec.load_demand"]; f["feedwater_temperature"] = one * 227.0
    f["cooling_water_inlet_temp"] = members["sec.cooling_water_temperature"]; f["cooling_water_outlet_temp"] = members["cond.cooling_water_outlet_temp"]
    # condenser/physics.py:692-693: outlet = inlet + rise, so the rise is their difference (to 1e-15 of the temperatures)
    f["condenser_cooling_water_temp_rise"] = members["cond.cooling_water_outlet_temp"] - members["sec.cooling_water_temperature"]
    # feedwater/physics.py:834: the configuration's auto_level_control, True unless a control command the step never issues clears it
    f["feedwater_auto_control"] = torch.ones_like(members["sec.cooling_water_temperature"])
    # the three values left over from inside the turbine step (secondary/__init__.py:955-958; include/npb.h NPB_INFO_TURBINE_*)
    f["turbine_efficiency"] = info["turbine_efficiency"]; f["turbine_hp_power"] = info["turbine_hp_power"]; f["turbine_lp_power"] = info["turbine_lp_power"]
    # condenser/physics.py:852-859: area factor (active / initial tubes, :122) x fouling factor x vacuum system efficiency, all end-of-step state
    area_factor = members["cond.active_tube_count"] / 84000.0
    fouling_factor = (1.0 - members["cond.total_fouling_resistance"] * 5).clamp_min(0.3)
    f["condenser_thermal_performance"] = area_factor * fouling_factor * members["cond.vacuum_system_efficiency"]
    return f


SECONDARY_RESULT_MEMBERS = ("sec.electrical_power_output", "sec.thermal_efficiency", "sec.sg_avg_temperature", "sec.sg_avg_quality",
                            "cond.heat_rejection_rate", "cond.vacuum_system_efficiency", "fw.running_mask", "fw.system_availability",
                            "chem.ph", "chem.water_aggressiveness", "chem.treatment_efficiency", "ph.controller_output",
                            "ph.pending_ammonia_dose", "ph.measured_ph", "sec.load_demand", "sec.cooling_water_temperature",
                            "cond.cooling_water_outlet_temp", "cond.active_tube_count", "cond.total_fouling_resistance")


FACTORY_DEFAULT_PUMP_THRESHOLDS = {"oil_level": {"threshold": 30.0, "comparison": "less_than", "action": "oil_top_off",
                                                 "cooldown_hours": 24.0, "priority": "HIGH"}}


class ConstantHeatSource:
    """systems/primary/reactor/heat_sources/constant_heat_source.py:29-102 (constructor and setpoint surface)."""

    def __init__(self, rated_power_mw: float = 3000.0, noise_enabled: bool = False, noise_std_percent: float = 5.0,
                 noise_seed: Optional[int] = None, noise_filter_time_constant: float = 30.0):
        self.rated_power_mw = rated_power_mw
        self.noise_enabled = noise_enabled
        self.noise_std_percent = noise_std_percent
        self.noise_seed = noise_seed
        self.noise_filter_time_constant = noise_filter_time_constant
        self.power_setpoint_percent = 100.0
        self._pending = None

    def set_power_setpoint(self, power_percent: float) -> None:
        self.power_setpoint_percent = float(np.clip(power_percent, 0.0, 150.0))
        self._pending = float(power_percent)


class HeatSource:
    """The reference's plugin interface for heat sources (heat_sources/heat_source_interface.py:23-112): subclass it and hand the
    object to NuclearPlantSimulator -- every step calls ``update(dt=..., reactor_state=..., control_action=...)`` on the host and
    feeds the returned ``thermal_power_mw`` / ``power_percent`` to the step as input columns (keys beyond those two --
    ``neutron_flux``, ``reactivity_pcm``, ``reactivity_components`` -- are not supported and raise).  Batches: compute the two
    columns yourself and call ``BatchedPlantEnv(heat_source="external").step(thermal_power_mw=..., power_percent=...)``."""

    def __init__(self, rated_power_mw: float = 3000.0):
        self.rated_power_mw = rated_power_mw
        self.current_power_mw = 0.0
        self.power_setpoint_percent = 100.0

    def update(self, dt: float, **kwargs) -> dict:
        raise NotImplementedError

    def set_power_setpoint(self, power_percent: float) -> None:
        self.power_setpoint_percent = power_percent

    def reset(self) -> None:
        pass


class ReactorHeatSource:
    """systems/primary/reactor/heat_sources/reactor_heat_source.py (point-kinetics heat source)."""

    def __init__(self, rated_power_mw: float = 3000.0):
        self.rated_power_mw = rated_power_mw
        self._pending = None


class _Namespace:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _PathProxy:
    """Read / write the plant's state through the reference's own attribute paths:
    ``sim.secondary_physics.feedwater_system.pump_system.pumps['FWP-1'].lubrication_system.oil_level`` resolves, step by
    step, against the reference attribute path every schema member carries (include/npb_fields.h), so code that reads
    or pokes the reference's object tree runs unchanged.  Only attributes that are state members exist; anything else
    raises AttributeError (there is no Python object tree behind this)."""

    def __init__(self, env, prefix, extras=None):
        object.__setattr__(self, "_env", env)
        object.__setattr__(self, "_prefix", prefix)
        object.__setattr__(self, "_extras", extras or {})

    @staticmethod
    def _index():
        idx = getattr(_PathProxy, "_paths", None)
        if idx is None:
            idx = {}
            for kind, slot, label, path in SCHEMA.columns():
                if path and not path.startswith("="):
                    idx[path] = (kind, slot)
            _PathProxy._paths = idx
        return idx

    def _resolve(self, path):
        idx = self._index()
        if path in idx:
            kind, slot = idx[path]
            v = self._env._get_slot(kind, slot)[0].item()
            return v if kind == "f64" else int(v)
        if any(p.startswith(path + ".") or p.startswith(path + "[") for p in idx):
            return _PathProxy(self._env, path)
        raise AttributeError("%s is not a state member of the plant" % path)

    # the two objects of the reference whose perform_maintenance is on the device: a feedwater pump and its lubrication system
    _MAINTAINABLE = re.compile(r"^secondary_physics\.feedwater_system\.pump_system\.pumps\['(FWP-[1-4])'\](\.lubrication_system)?$")

    def _perform_maintenance(self, pump_id):
        env = self._env

        def perform_maintenance(maintenance_type="general", **kwargs):
            """FeedwaterPump.perform_maintenance / FeedwaterPumpLubricationSystem.perform_maintenance (pump_system.py:750,
            pump_lubrication.py:625) on this pump, now.  Returns ``{'success': bool}``: the remaining keys of the reference's result
            dict (duration_hours, work_performed, findings, effectiveness_score ...) are omitted.  A maintenance type the action
            catalog does not know is the reference's "Unknown maintenance type": success False, nothing changed."""
            names = _lib.MAINT_ACTION_NAMES
            if maintenance_type not in names:
                return {"success": False}
            cid = kwargs.get("component_id")
            if cid is None or isinstance(cid, str):      # a component_id that names no bearing: "Invalid bearing component" (-1 on the device)
                cid = _lib.MAINT_BEARINGS.get(cid, -1)
            ok = env.perform_maintenance(names.index(maintenance_type), pump_id, bearing=cid, target_level=kwargs.get("target_level"))
            return {"success": bool(ok[0].item())}
        return perform_maintenance

    # ... and the four whose perform_maintenance is npb_perform_component_maintenance: the steam-generator system, one of its
    # generators, the condenser, one of its steam-jet ejectors
    _VACUUM_SYSTEM = "secondary_physics.condenser.vacuum_system"
    _COMPONENTS = ((re.compile(r"^secondary_physics\.steam_generator_system\.steam_generators\[([0-2])\]$"), "steam_generator"),
                   (re.compile(r"^secondary_physics\.steam_generator_system$"), "steam_generator_system"),
                   (re.compile(r"^secondary_physics\.condenser$"), "condenser"),
                   (re.compile(r"^secondary_physics\.condenser\.vacuum_system\.ejectors\['(SJE-00[12])'\]$"), "ejector"))

    def _perform_component_maintenance(self, component, unit):
        env = self._env

        def perform_maintenance(maintenance_type=None, **kwargs):
            """SteamGenerator / EnhancedSteamGeneratorPhysics / EnhancedCondenserPhysics / SteamJetEjector.perform_maintenance on this
            object, now (BatchedPlantEnv.perform_component_maintenance).  Returns ``{'success': bool}``; kwargs as the reference's:
            ``cleaning_type``, ``sg_index`` (the system delegates a generator's maintenance type to that generator).  A type the
            catalog does not know is the reference's "Unknown maintenance type" (success False, nothing changed) -- on an ejector
            it is the dispatcher's general maintenance, as there.  A handler that is not offered raises ValueError."""
            comp, k = component, unit
            if (comp, maintenance_type) in _lib.COMPONENT_ACTIONS_NOT_OFFERED:
                _lib.component_action_index(comp, maintenance_type)
            if (comp, maintenance_type) not in _lib.COMPONENT_ACTIONS:
                sg_index = kwargs.get("sg_index")
                if comp == "ejector":
                    maintenance_type = "general"
                elif comp == "steam_generator_system" and sg_index is not None and 0 <= sg_index < 3:
                    comp, k = "steam_generator", int(sg_index)
                    if (comp, maintenance_type) in _lib.COMPONENT_ACTIONS_NOT_OFFERED:
                        _lib.component_action_index(comp, maintenance_type)
                if (comp, maintenance_type) not in _lib.COMPONENT_ACTIONS:
                    return {"success": False}
            ok = env.perform_component_maintenance(comp, maintenance_type, unit=k, cleaning_type=kwargs.get("cleaning_type"),
                                                   tubes_to_plug=kwargs.get("tubes_to_plug"))
            return {"success": bool(ok[0].item())}
        return perform_maintenance

    def __getattr__(self, name):
        extras = object.__getattribute__(self, "_extras")
        if name in extras:
            return extras[name]
        if name == "perform_maintenance":
            m = self._MAINTAINABLE.match(self._prefix or "")
            if m:
                return self._perform_maintenance(m.group(1))
            for pattern, component in self._COMPONENTS:
                m = pattern.match(self._prefix or "")
                if m:
                    unit = 0 if not m.groups() else int(m.group(1)) if component == "steam_generator" else _lib.EJECTOR_IDS.index(m.group(1))
                    return self._perform_component_maintenance(component, unit)
        if name == "ejectors" and self._prefix == self._VACUUM_SYSTEM:     # its members are no plain paths of the schema
            return _PathProxy(self._env, self._prefix + ".ejectors")
        return self._resolve("%s.%s" % (self._prefix, name) if self._prefix else name)

    def __getitem__(self, key):
        if self._prefix == self._VACUUM_SYSTEM + ".ejectors" and key in _lib.EJECTOR_IDS:
            return _PathProxy(self._env, "%s[%r]" % (self._prefix, key))
        return self._resolve("%s[%r]" % (self._prefix, key))

    def _assign(self, path, value):
        idx = self._index()
        if path not in idx:
            raise AttributeError("%s is not a state member of the plant" % path)
        kind, slot = idx[path]
        self._env._set_slot(kind, slot, [value])

    def __setattr__(self, name, value):
        self._assign("%s.%s" % (self._prefix, name), value)

    def __setitem__(self, key, value):
        self._assign("%s[%r]" % (self._prefix, key), value)


class NuclearPlantSimulator:
    """Single-plant facade with the reference's signatures (simulator/core/sim.py:27-258), so that loops written
    against the reference -- ``sim.primary_physics.heat_source.set_power_setpoint(p); sim.step(action=...)``
    (maintenance_scenario_runner.py:383-411, 651-671) -- run unchanged on one lane of the HIP stepper.

    Differences, all explicit: ``enable_state_management=True`` (the reference's default, sim.py:31) turns on what the
    path needs of it -- the automatic maintenance of the feedwater pumps, with the priority delays of the configuration's
    ``maintenance_system.maintenance_mode`` (aggressive / ultra_aggressive: none; anything else: 1 h / 4 h / 24 h,
    sim.py:97-128, auto_maintenance.py:187-198) and the feedwater thresholds of
    ``maintenance_system.component_configs.feedwater.thresholds`` when the configuration has them -- not the pandas state
    log; ``secondary_config`` is honoured for the
    initial-condition keys nuclear_sim_amd.scenarios can map (others are listed in ``ignored_initial_conditions``);
    ``reset()`` follows the reference's own reset (default configuration; pinned by tests/golden/r1_*.npz)."""

    def __init__(self, dt: float = 1.0, heat_source=None, enable_secondary: bool = True,
                 enable_state_management: bool = True, max_state_rows: int = 100000, secondary_config=None,
                 secondary_config_file: Optional[str] = None, device: int = 0):
        if secondary_config is None and secondary_config_file is not None and enable_secondary:
            secondary_config = self._load_config_file(secondary_config_file)
        if heat_source is None or heat_source == "reactor":
            heat_source = ReactorHeatSource()            # sim.py:41-44: the default heat source is the reactor model
        elif heat_source == "constant":
            heat_source = ConstantHeatSource(noise_std_percent=0.1)
        constant = isinstance(heat_source, ConstantHeatSource)
        # anything else must speak the reference's HeatSource plugin interface; an object this facade cannot map is refused
        # rather than silently run as the reactor model
        plugin = not constant and not isinstance(heat_source, ReactorHeatSource)
        if plugin and not (callable(getattr(heat_source, "update", None)) and hasattr(heat_source, "rated_power_mw")):
            raise TypeError("heat_source must be a ConstantHeatSource, a ReactorHeatSource, 'constant', 'reactor' or an object with the "
                            "reference's HeatSource interface (update(dt, **kwargs) -> {'thermal_power_mw', 'power_percent'}, "
                            "rated_power_mw): got %r" % (heat_source,))
        self._plugin = heat_source if plugin else None
        self.dt = dt
        self.enable_secondary = bool(enable_secondary)
        self.enable_state_management = enable_state_management
        # StateManager's clock (state_manager.py:51-52,82-109): a random start date drawn from the `random` module, advanced
        # by dt minutes per step, never put back by reset(); without state management info["datetime"] is None
        self._datetime = None
        if enable_state_management:
            import datetime as _dt
            import random as _random
            self._datetime = _dt.datetime(_random.randint(2020, 2030), _random.randint(1, 12), _random.randint(1, 28),
                                          _random.randint(0, 23), _random.randint(0, 59), 0)
        params = {"rated_power_mw": float(heat_source.rated_power_mw)}
        if constant:
            params["hs_noise_filter_tau"] = float(heat_source.noise_filter_time_constant)
        maint_cfg = (secondary_config or {}).get("maintenance_system", {}) if isinstance(secondary_config, dict) else {}
        # sim.py:97-128, auto_maintenance.py:187-198: anything but an aggressive mode in the configuration -- no configuration at
        # all included -- delays execution by priority
        if maint_cfg.get("maintenance_mode") not in ("aggressive", "ultra_aggressive") and enable_state_management:
            params.update(maint_start_delay_hours=1.0, maint_medium_delay_hours=4.0, maint_low_delay_hours=24.0)
        thresholds = ((maint_cfg.get("component_configs") or {}).get("feedwater") or {}).get("thresholds")
        if thresholds is None:
            # no maintenance configuration: the state manager's factory default (state_manager.py
            # _create_default_maintenance_config) gives a feedwater pump this one threshold -- not the data-gen action-test
            # table, which would top a pump off at 58 % (fixture m14_default_configuration_maintenance)
            thresholds = dict(FACTORY_DEFAULT_PUMP_THRESHOLDS)
        self._env = BatchedPlantEnv(1, dt=dt, heat_source="constant" if constant else ("external" if plugin else "reactor"),
                                    noise_enabled=bool(constant and heat_source.noise_enabled),
                                    noise_std_percent=float(heat_source.noise_std_percent) if constant else 0.1,
                                    noise_seeds=[heat_source.noise_seed] if (constant and heat_source.noise_enabled and
                                                                             heat_source.noise_seed is not None) else None,
                                    device=device, maintenance=bool(enable_state_management and enable_secondary), params=params,
                                    maintenance_thresholds=thresholds, mode="full" if enable_secondary else "primary",
                                    reactivity_components=not constant and not plugin)
        # the reference's object tree, as far as it is plant state: attribute paths resolve against the schema
        self.primary_physics = _PathProxy(self._env, "primary_physics",
                                          extras={"heat_source": heat_source, "rated_power_mw": heat_source.rated_power_mw})
        self.secondary_physics = _PathProxy(self._env, "secondary_physics") if enable_secondary else None
        self.ignored_initial_conditions = []
        if secondary_config is not None and enable_secondary:
            self._apply_secondary_config(secondary_config)
        self.load_demand = 100.0
        self.cooling_water_temp = 25.0

    def _apply_secondary_config(self, cfg: dict) -> None:
        """initial_conditions of the composed configuration -> state columns (nuclear_sim_amd.scenarios)"""
        from . import scenarios
        sec = cfg.get("secondary_system", cfg)
        fields = {}
        fw_ic = dict(sec.get("feedwater", {}).get("initial_conditions", {}) or {})
        known = set(scenarios.FEEDWATER_IC_DEFAULTS)
        self.ignored_initial_conditions += ["feedwater." + k for k in fw_ic if k not in known]
        self._feedwater_ic = {k: v for k, v in fw_ic.items() if k in known}
        if fw_ic:
            eff = float(self._env.get_field("pump.lubrication_effectiveness")[0].item())
            fields.update(scenarios.feedwater_fields({k: v for k, v in fw_ic.items() if k in known}, 1, eff))
        sg_ic = sec.get("steam_generator", {}).get("initial_conditions", {}) or {}
        if "sg_steam_flows" in sg_ic:
            for k in range(scenarios.NUM_SG):
                fields[("sg.steam_flow_rate", k)] = np.array([float(sg_ic["sg_steam_flows"][k])])
        self.ignored_initial_conditions += ["steam_generator." + k for k in sg_ic if k != "sg_steam_flows"]
        tb_ic = sec.get("turbine", {}).get("initial_conditions", {}) or {}
        if "rotor_temperature" in tb_ic:
            fields["turb.rotor_temperature"] = np.array([float(tb_ic["rotor_temperature"])])
        if "bearing_temperatures" in tb_ic:
            for k in range(4):
                fields[("turb.bearing_metal_temp", 0, k)] = np.array([float(tb_ic["bearing_temperatures"][k])])
        self.ignored_initial_conditions += ["turbine." + k for k in tb_ic if k not in ("rotor_temperature", "bearing_temperatures")]
        self.ignored_initial_conditions += ["condenser." + k for k in (sec.get("condenser", {}).get("initial_conditions", {}) or {})]
        self._env.set_fields(fields)

    @property
    def state(self):
        """ReactorState view of the primary columns (sim.state, sim.py:85,151): attribute name -> current value"""
        out = {}
        for sec, f in (SCHEMA.by_name[k] for k in SCHEMA.by_name if k.startswith("prim.")):
            if f.count == 1 and f.path.startswith("primary_physics.state."):
                out[f.path[len("primary_physics.state."):]] = self._env.get_field("prim." + f.name)[0].item()
        return _Namespace(**out)

    def _state_after_actuators(self, a: int, magnitude: float):
        """``self.state`` with this step's actuator movement applied: PrimaryReactorPhysics._apply_control_actions
        (primary/__init__.py:289-359; rates :174-176 and the 50 ppm/s of :333,341; which action moves what: sim.py:260-288) -- what a
        HeatSource plugin is shown, since the reference moves the actuators before it updates the heat source."""
        st = self.state
        p, dt = self._env.params, self.dt
        if a == ControlAction.CONTROL_ROD_INSERT.value:
            st.control_rod_position = max(0, st.control_rod_position - p.max_control_rod_speed * dt * magnitude)
        elif a == ControlAction.CONTROL_ROD_WITHDRAW.value:
            st.control_rod_position = min(100, st.control_rod_position + p.max_control_rod_speed * dt * magnitude)
        elif a == ControlAction.INCREASE_COOLANT_FLOW.value:
            st.coolant_flow_rate = min(50000, st.coolant_flow_rate + p.max_flow_change_rate * dt * magnitude)
        elif a == ControlAction.DECREASE_COOLANT_FLOW.value:
            st.coolant_flow_rate = max(5000, st.coolant_flow_rate - p.max_flow_change_rate * dt * magnitude)
        elif a == ControlAction.DILUTE_BORON.value:
            st.boron_concentration = max(0, st.boron_concentration - 50.0 * dt * magnitude)
        elif a == ControlAction.BORATE_COOLANT.value:
            st.boron_concentration = min(3000, st.boron_concentration + 50.0 * dt * magnitude)
        elif a == ControlAction.OPEN_STEAM_VALVE.value:
            st.steam_valve_position = min(100, st.steam_valve_position + p.max_valve_speed * dt * magnitude)
        elif a == ControlAction.CLOSE_STEAM_VALVE.value:
            st.steam_valve_position = max(0, st.steam_valve_position - p.max_valve_speed * dt * magnitude)
        return st

    def set_power_setpoint(self, power_percent: float) -> None:
        """heat_source.set_power_setpoint  constant_heat_source.py:93-102 (applied at the next step)."""
        if self._plugin is not None:
            self._plugin.set_power_setpoint(float(power_percent))
        else:
            self.primary_physics.heat_source._pending = float(power_percent)

    def step(self, action: Optional[ControlAction] = None, magnitude: float = 1.0, load_demand: float = None,
             cooling_water_temp: float = None) -> Dict:
        a = ControlAction.NO_ACTION.value if action is None else (action.value if isinstance(action, ControlAction) else int(action))
        hs = self.primary_physics.heat_source
        if self._plugin is not None:
            # primary/__init__.py:200-207: _apply_control_actions FIRST, then heat_source.update(dt, reactor_state, control_action) -- the
            # plugin sees the rods, flow, boron and valve where this step's action has moved them.  The launch moves them too (its
            # result is an input column of the launch), so the view handed to the plugin is moved here, on the host, by the same rule
            res = self._plugin.update(dt=self.dt, reactor_state=self._state_after_actuators(a, float(magnitude)), control_action=ControlAction(a))

            def given(v):           # a key the plugin filled in (None, an empty dict, a zero -- of any numeric type -- count as absent)
                if v is None or (isinstance(v, dict) and not v):
                    return False
                return not (np.isscalar(v) and float(v) == 0.0) if not isinstance(v, dict) else True
            unsupported = [k for k in ("neutron_flux", "reactivity_pcm", "reactivity_components") if k in res and given(res[k])]
            if unsupported:
                raise NotImplementedError("a HeatSource plugin's result may carry thermal_power_mw and power_percent; %s are not supported" % unsupported)
            obs, rew, done, info = self._env.step(action=[a], magnitude=[magnitude], thermal_power_mw=[float(res["thermal_power_mw"])],
                                                  power_percent=[float(res["power_percent"])],
                                                  cooling_water_temp=None if cooling_water_temp is None else [cooling_water_temp])
        else:
            sp, hs._pending = getattr(hs, "_pending", None), None
            obs, rew, done, info = self._env.step(action=[a], magnitude=[magnitude],
                                                  power_setpoint=None if sp is None else [sp],
                                                  cooling_water_temp=None if cooling_water_temp is None else [cooling_water_temp])
        o = obs[0].cpu().numpy().copy()
        rho = info.pop("reactivity_components", None)
        inf = {k: (v[0].item()) for k, v in info.items()}
        inf["scram_activated"] = bool(inf["scram_activated"])
        # sim.py:205: the reactor model's ten terms in pcm; ConstantHeatSource has none (primary/__init__.py:225)
        inf["reactivity_components"] = {} if rho is None else {k: float(v[0].item()) for k, v in rho.items()}
        if self._datetime is not None:
            import datetime as _dt
            self._datetime += _dt.timedelta(minutes=self.dt)
        inf["datetime"] = self._datetime.isoformat() if self._datetime is not None else None
        if not self.enable_secondary:   # sim.py:199-206,225: without a secondary side the dict has the primary keys only
            inf = {k: inf[k] for k in ("time", "datetime", "thermal_power", "scram_activated", "reactivity", "reactivity_components", "trip_flags")}
            o = o[:12]
        else:
            inf["secondary_system"] = self._secondary_result()
        return {"observation": o, "reward": float(rew[0].item()), "done": bool(done[0].item()), "info": inf}

    @staticmethod
    def _load_config_file(path: str) -> dict:
        """SecondaryReactorPhysics(config_file=...)  secondary/__init__.py:181-205: a YAML file, its ``secondary_system``
        section when it has one; the comprehensive configuration's ``maintenance_system`` section rides along"""
        import yaml
        with open(path, "r") as fh:
            data = yaml.safe_load(fh)
        cfg = dict(data.get("secondary_system", data))
        if "maintenance_system" in data and "maintenance_system" not in cfg:
            cfg["maintenance_system"] = data["maintenance_system"]
        return cfg

    def _secondary_result(self) -> Dict[str, float]:
        """info["secondary_system"]: every scalar key of the reference's result dict (secondary/__init__.py:922-1010) that is a
        function of what the step produces -- all 56 scalars (turbine_efficiency, turbine_hp_power and turbine_lp_power are the
        step's info columns NPB_INFO_TURBINE_*; condenser_thermal_performance is end-of-step state)."""
        return {k: float(v[0].item()) for k, v in self._env.secondary_result().items()}

    def reset(self, start_at_steady_state: bool = True):
        """sim.py:546-581: the reference's reset (not a re-construction); the configured feedwater initial conditions
        are re-applied as EnhancedFeedwaterPhysics.reset does (feedwater/physics.py:1286-1323)."""
        env = self._env
        obs = env.reset(reference=True, start_at_steady_state=start_at_steady_state)
        if getattr(self, "_feedwater_ic", None):
            from . import scenarios
            eff = torch.stack([env.get_field("pump.lubrication_effectiveness", instance=k) for k in range(scenarios.NUM_PUMPS)], dim=1).cpu().numpy()
            env.set_fields(scenarios.feedwater_reset_fields(self._feedwater_ic, 1, eff, start_at_steady_state))
            obs = env.get_observation()
        if self._plugin is not None:
            self._plugin.reset()        # primary/__init__.py reset_system -> heat_source.reset()
        else:
            self.primary_physics.heat_source._pending = None
        if hasattr(self.primary_physics.heat_source, "power_setpoint_percent"):
            self.primary_physics.heat_source.power_setpoint_percent = 100.0
        self.load_demand = 100.0
        self.cooling_water_temp = 25.0
        return obs[0].cpu().numpy().copy()[: 22 if self.enable_secondary else 12]

    def get_observation(self) -> np.ndarray:
        return self._env.get_observation()[0].cpu().numpy().copy()[: 22 if self.enable_secondary else 12]


class NuclearPlantEnv:
    """Gym-style wrapper  sim.py:911-940."""

    def __init__(self, **kw):
        self.sim = NuclearPlantSimulator(**kw)
        self.action_space_size = len(ControlAction)
        self.observation_space_size = 22 if self.sim.enable_secondary else 12   # sim.py:917-918

    def render(self):
        return None

    def reset(self):
        return self.sim.reset()

    def step(self, action_idx: int, load_demand: float = None, cooling_water_temp: float = None):
        r = self.sim.step(ControlAction(action_idx), load_demand=load_demand, cooling_water_temp=cooling_water_temp)
        return r["observation"], r["reward"], r["done"], r["info"]
