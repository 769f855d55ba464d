"""Reference power-profile fixtures: tests/golden/power_profile/<case>.npz.

Runs the REFERENCE's own MaintenanceScenarioRunner._generate_power_profile and ._set_target_power (needs a machine with the reference;
oracle/ref_harness/refsim puts it on the path) on runner objects made with object.__new__ -- no simulator is built: the runner gets a
config dict with one load profile and a stand-in simulator whose heat source is a real ConstantHeatSource, so the setpoints recorded are
what its set_power_setpoint (with its clip) stored.  Per case (one load profile = base_power_percent / noise_std_percent), per horizon T
and per seed: np.random.seed(seed), then TWO runners in a row on the global stream, each drawing its profile of T steps and ramping
through it from a fresh start.  Written per horizon: target_<T> and setpoint_<T> as [2, T, seeds] float64, and the global stream's
state after both (pos, has_gauss, cached gaussian, CRC-32 of the 624-word key) -- what RandomState(seed) holds after 2 T normals.

    python tools/make_power_profile_golden.py
"""
import os
import sys
import types
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEEDS = (0, 1, 3, 42, 12345, 2 ** 32 - 1)
HORIZONS = (1, 2, 3, 4, 48, 60, 333)
#        case               base_power_percent, noise_std_percent
CASES = {"steady_98_0p2": (98.0, 0.2),          # the template's second profile
         "clipped_104p9_2p0": (104.9, 2.0),     # the upper clip engages (seed 3, T = 60: 17 raw values)
         "floor_20p05_0p1": (20.05, 0.1),       # the lower clip engages
         "noiseless_90_0": (90.0, 0.0),
         "composer_90_2p0": (90.0, 2.0)}        # what the composer writes for an action test


def run_runner(Runner, heat_source, base, std, T):
    """one runner: its profile of T steps and the setpoints its ramp hands the heat source"""
    r = object.__new__(Runner)
    r.config = {"simulation_config": {"scenario": "fixture"},
                "load_profiles": {"profiles": {"fixture": {"base_power_percent": base, "noise_std_percent": std}}}}
    r.simulator = types.SimpleNamespace(primary_physics=types.SimpleNamespace(heat_source=heat_source))
    target = np.array(r._generate_power_profile(T), dtype=np.float64)
    setpoint = np.empty(T)
    for i in range(T):
        r._set_target_power(target[i])
        setpoint[i] = heat_source.power_setpoint_percent
    return target, setpoint


def main():
    from oracle.ref_harness import refsim
    refsim.setup()
    np.random.normal = refsim._REAL_NORMAL         # the harness flattens it for the pH controller; the profile is what is recorded here
    with refsim.quiet():
        from data_gen.runners.maintenance_scenario_runner import MaintenanceScenarioRunner
        from systems.primary.reactor.heat_sources import ConstantHeatSource
    out_dir = os.path.join(ROOT, "tests", "golden", "power_profile")
    os.makedirs(out_dir, exist_ok=True)
    for case, (base, std) in CASES.items():
        arrays = {"seeds": np.array(SEEDS, dtype=np.int64), "horizons": np.array(HORIZONS, dtype=np.int64),
                  "base_power_percent": np.float64(base), "noise_std_percent": np.float64(std)}
        clipped = 0
        for T in HORIZONS:
            target, setpoint = np.empty((2, T, len(SEEDS))), np.empty((2, T, len(SEEDS)))
            pos, has, cached, crc = [], [], [], []
            for j, seed in enumerate(SEEDS):
                np.random.seed(seed)
                for run in range(2):
                    target[run, :, j], setpoint[run, :, j] = run_runner(MaintenanceScenarioRunner, ConstantHeatSource(), base, std, T)
                st = np.random.get_state()
                pos.append(st[2]); has.append(st[3]); cached.append(st[4]); crc.append(zlib.crc32(np.ascontiguousarray(st[1], dtype=np.uint32).tobytes()))
            arrays.update({"target_%d" % T: target, "setpoint_%d" % T: setpoint, "state_pos_%d" % T: np.array(pos, dtype=np.int32),
                           "state_has_gauss_%d" % T: np.array(has, dtype=np.int32), "state_cached_%d" % T: np.array(cached),
                           "state_key_crc32_%d" % T: np.array(crc, dtype=np.uint32)})
            clipped += int(np.sum((target == 105.0) | (target == 20.0)))
        path = os.path.join(out_dir, case + ".npz")
        np.savez_compressed(path, **arrays)
        print("%-20s base %6.2f std %4.2f  %d horizons x %d seeds x 2 runners, %d targets on a clip bound -> %s (%d bytes)" % (
            case, base, std, len(HORIZONS), len(SEEDS), clipped, os.path.relpath(path, ROOT), os.path.getsize(path)))


if __name__ == "__main__":
    main()
