"""When does a maintenance action first fire?  The data-gen timing optimiser's question, answered for a whole batch of probes at once.

The reference's ``TimingOptimizer._test_trigger_timing`` builds one simulator for one parameter value, steps it until the target action's
work order appears and returns that time (optimization/timing_optimizer.py:273-320); ``_binary_search_parameter`` runs up to ten such
simulations one after the other to move the time onto a target (:121-195).  Here one batch holds every probe value: the plants are the
same action-test scenario (``BatchedPlantEnv.action_test``) with one state field overridden per plant, the device's work-order summary
(``enable_maintenance_summary``) records per plant when the action's first work order was created and completed, and the only thing
the host reads while the batch runs is one flag every 32 steps.  ``sweep`` is the optimiser's search as grid refinement over such
batches, and ``banked_trigger_times`` streams M scenarios through fewer lanes with the start bank and the episode records.  It does not restate the reference's walk through configuration paths or its table of parameter bounds: the caller names the
state field and the interval.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

CHECK_EVERY = 32      # steps between two looks at "has every plant fired?" (one .item() each)


def trigger_times(action: str, seeds: Sequence[int], hours: float, dt: float = 1.0, fields: Optional[dict] = None,
                  values: Optional[Sequence[float]] = None, power_setpoint: float = 90.0, unit: Optional[int] = None, device: int = 0,
                  randomize: bool = True, params: Optional[dict] = None, storage: str = "f64", keep_log: bool = False,
                  return_env: bool = False) -> Dict[str, np.ndarray]:
    """First-created and first-completed times [hours, plant clock] of ``action``'s work orders in ``action_test(action, seeds, dt)``
    plants stepped for ``int(hours * 60 / dt)`` steps of ``dt`` minutes, NaN where the action never fired.

    ``fields`` overrides state members before the first step, as ``BatchedPlantEnv.set_fields`` takes them: a dict from a field name or
    ``(name, instance[, k])`` to an ``[n]`` array; ``values`` is shorthand for one override, ``{fields: values}`` with ``fields`` the one
    key.  ``unit`` restricts the key to one pump (None = any).  ``power_setpoint`` is held for the whole run, as the optimiser's probe
    runs hold theirs.  The run stops early once every plant has fired (looked at every ``CHECK_EVERY`` steps).  Returns
    ``{"first_created_hours", "first_completed_hours", "n_created", "n_completed", "steps", "dropped"}``; with ``return_env`` also the
    env under ``"env"`` (the caller closes it), else it is closed."""
    import torch
    from .env import BatchedPlantEnv
    n = len(seeds)
    env = BatchedPlantEnv.action_test(action, seeds, dt=dt, device=device, randomize=randomize, params=params, storage=storage)
    try:
        if values is not None:
            if fields is None or isinstance(fields, dict):
                raise ValueError("values needs fields to be the one field it overrides")
            fields = {fields: values}
        if fields:
            env.set_fields({k: np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for k, v in fields.items()})
        env.enable_maintenance_summary([("feedwater", action, unit)], keep_log=keep_log)
        S = env.maintenance_summary()
        sp = torch.full((n,), float(power_setpoint), dtype=torch.float64, device=env.device)
        steps, total = 0, int(hours * 60 / dt)
        while steps < total:
            env.step(power_setpoint=sp)
            steps += 1
            if steps % CHECK_EVERY == 0 and bool(torch.isfinite(S["first_created"]).all().item()):
                break
        created = S["first_created"][0].cpu().numpy() / 60.0
        completed = S["first_completed"][0].cpu().numpy() / 60.0
        out = {"first_created_hours": np.where(np.isfinite(created), created, np.nan),
               "first_completed_hours": np.where(np.isfinite(completed), completed, np.nan),
               "n_created": S["n_created"][0].cpu().numpy(), "n_completed": S["n_completed"][0].cpu().numpy(),
               "steps": steps, "dropped": int(S["dropped"].item())}
        if return_env:
            out["env"] = env
        return out
    finally:
        if not return_env:
            env.close()


def sweep(action: str, seed: int, field, lo: float, hi: float, target_hours: float, tolerance_hours: float, points: int = 64,
          rounds: int = 3, dt: float = 1.0, **kw) -> Dict[str, object]:
    """The timing optimiser's search as grid refinement: which value of state field ``field`` (a name or ``(name, instance[, k])``) in
    ``[lo, hi]`` makes ``action`` first fire closest to ``target_hours`` in scenario ``seed``?  Each round is one batch of ``points``
    probe values spread evenly over the interval, every plant the same scenario seed, stepped for ``2 * target_hours`` as the
    reference's probe runs are; the next round's interval is the bracket around the probe closest to the target (its two grid
    neighbours).  Stops after ``rounds`` rounds, or as soon as a probe is within ``tolerance_hours``.  Returns ``{"value", "hours",
    "error_hours", "converged", "rounds", "probes"}``: the best probe's value and first-created time, and ``probes``, an ``[m, 3]`` array
    of (round, value, first-created hours; NaN = never fired) of every probe run.  ``value`` is None if no probe ever fired."""
    if points < 3:
        raise ValueError("a sweep needs at least 3 points per round")
    lo, hi = float(lo), float(hi)
    probes, best = [], None
    done = 0
    for r in range(int(rounds)):
        values = np.linspace(lo, hi, int(points))
        t = trigger_times(action, [int(seed)] * len(values), 2.0 * float(target_hours), dt=dt, fields=field, values=values, **kw)["first_created_hours"]
        probes += [(r, float(v), float(h)) for v, h in zip(values, t)]
        done = r + 1
        err = np.abs(t - float(target_hours))
        if np.all(np.isnan(err)):
            break
        j = int(np.nanargmin(err))
        if best is None or err[j] < best[2]:
            best = (float(values[j]), float(t[j]), float(err[j]))
        if best[2] <= float(tolerance_hours):
            break
        lo, hi = float(values[max(j - 1, 0)]), float(values[min(j + 1, len(values) - 1)])
    return {"value": None if best is None else best[0], "hours": None if best is None else best[1],
            "error_hours": None if best is None else best[2], "converged": best is not None and best[2] <= float(tolerance_hours),
            "rounds": done, "probes": np.array(probes, dtype=np.float64).reshape(-1, 3)}


def banked_trigger_times(action: str, seeds: Sequence[int], hours: float, lanes: int, dt: float = 1.0, unit: Optional[int] = None,
                         power_setpoint: float = 90.0, device: int = 0, randomize: bool = True, params: Optional[dict] = None,
                         storage: str = "f64", capacity: Optional[int] = None) -> Dict[str, np.ndarray]:
    """``trigger_times`` for M = ``len(seeds)`` scenarios streamed through ``lanes`` <= M plants: one env whose start bank holds the M
    scenarios (``action_test(..., bank_seeds=seeds, autoreset=True, max_episode_steps=int(hours * 60 / dt), noise_generator="device",
    episode_streams=True)``, slots ``arange(lanes) % M`` advancing by ``lanes``), a work-order summary of one key, and episode records that
    carry each finished episode's summary rows and clear them (``enable_episode_records``).  Every episode that starts from bank entry s
    is the run a fresh env of ``seeds[s]`` makes, so its record is that scenario's answer.

    Each plant's first episode runs before its first restart from the bank; those records (``start == -1``) are ignored.  Plant p then
    takes entries p, p + lanes, ... and no episode is longer than ``max_episode_steps``, so after ``(1 + ceil(M / lanes)) *
    max_episode_steps`` steps every entry has a finished episode: the run stops there without ever reading a flag back.  The records are
    drained once per ``max_episode_steps`` steps.  Where terminations let an entry be played more than once, its first record (by step,
    then plant) is taken.

    Returns, per seed, ``trigger_times``' keys -- ``first_created_hours`` / ``first_completed_hours`` (the summary's plant-clock minutes
    / 60, NaN = never), ``n_created``, ``n_completed``, and ``steps`` (here: steps the env ran), ``dropped`` -- plus ``length`` (the
    episode's steps) and ``terminated`` (it ended by a scram rather than by the step limit)."""
    import torch
    from .env import BatchedPlantEnv
    seeds = [int(s) for s in seeds]
    M, lanes = len(seeds), int(lanes)
    if not 1 <= lanes <= M:
        raise ValueError("lanes must be 1 .. len(seeds) = %d, not %d" % (M, lanes))
    L = int(hours * 60 / dt)
    if L < 1:
        raise ValueError("hours * 60 / dt must be at least one step")
    env = BatchedPlantEnv.action_test(action, seeds[:lanes], dt=dt, device=device, randomize=randomize, params=params, storage=storage,
                                      bank_seeds=seeds, autoreset=True, max_episode_steps=L, noise_generator="device", episode_streams=True)
    try:
        env.enable_maintenance_summary([("feedwater", action, unit)])
        env.enable_episode_records(capacity, summary=True, clear_summary=True)
        sp = torch.full((lanes,), float(power_setpoint), dtype=torch.float64, device=env.device)
        total = (1 + -(-M // lanes)) * L
        out = {"first_created_hours": np.full(M, np.nan), "first_completed_hours": np.full(M, np.nan),
               "n_created": np.zeros(M, dtype=np.int32), "n_completed": np.zeros(M, dtype=np.int32),
               "length": np.zeros(M, dtype=np.int32), "terminated": np.zeros(M, dtype=bool)}
        seen = np.zeros(M, dtype=bool)

        def drain():
            rec = env.episode_records()
            for k in np.flatnonzero(rec["start"] >= 0):      # sorted by (step, plant): an entry's first record wins
                s = int(rec["start"][k])
                if seen[s]:
                    continue
                seen[s] = True
                created, completed = rec["first_created"][k, 0] / 60.0, rec["first_completed"][k, 0] / 60.0
                out["first_created_hours"][s] = created if np.isfinite(created) else np.nan
                out["first_completed_hours"][s] = completed if np.isfinite(completed) else np.nan
                out["n_created"][s], out["n_completed"][s] = rec["n_created"][k, 0], rec["n_completed"][k, 0]
                out["length"][s], out["terminated"][s] = rec["length"][k], rec["terminated"][k]
        for step in range(1, total + 1):
            env.step(power_setpoint=sp)
            if step % L == 0:
                drain()
        if not seen.all():
            raise RuntimeError("banked_trigger_times: bank entries %r have no finished episode after %d steps" % (np.flatnonzero(~seen).tolist(), total))
        out["steps"] = total
        out["dropped"] = int(env.maintenance_summary()["dropped"].item())
        return out
    finally:
        env.close()
