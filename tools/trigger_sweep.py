"""Which value of a state field makes a maintenance action first fire at a target time?

    python tools/trigger_sweep.py --action oil_top_off --seed 7 --field pump.oil_level --instance 0 --lo 59.2 --hi 63.0 \
        --target-hours 3.0 --tolerance-hours 0.1 [--points 64] [--rounds 3] [--dt 5] [--unit 0] [--out sweep.json]

The command-line face of nuclear_sim_amd.timing.sweep: the data-gen timing optimiser's search (optimization/timing_optimizer.py:121-195,
273-320), each round one batch of --points probes of the same scenario seed instead of one simulation per probe.  Prints one JSON line:
the value, the time it fires at, whether that is within the tolerance, and every probe as [round, value, hours (null = never fired)].
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nuclear_sim_amd import timing  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--action", required=True)
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--field", required=True, help="state field, e.g. pump.oil_level")
    ap.add_argument("--instance", type=int, default=0, help="which pump / generator / ... the field belongs to")
    ap.add_argument("--k", type=int, default=0, help="element of an array member")
    ap.add_argument("--lo", type=float, required=True)
    ap.add_argument("--hi", type=float, required=True)
    ap.add_argument("--target-hours", type=float, required=True)
    ap.add_argument("--tolerance-hours", type=float, required=True)
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dt", type=float, default=1.0, help="minutes per step")
    ap.add_argument("--unit", type=int, default=None, help="count the action on this pump only")
    ap.add_argument("--power-setpoint", type=float, default=90.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = timing.sweep(a.action, a.seed, (a.field, a.instance, a.k), a.lo, a.hi, a.target_hours, a.tolerance_hours, points=a.points,
                     rounds=a.rounds, dt=a.dt, unit=a.unit, power_setpoint=a.power_setpoint)
    s["probes"] = [[int(r), v, None if h != h else h] for r, v, h in s["probes"].tolist()]
    s.update(action=a.action, seed=a.seed, field=[a.field, a.instance, a.k], target_hours=a.target_hours, tolerance_hours=a.tolerance_hours)
    line = json.dumps(s)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if s["converged"] else 1


if __name__ == "__main__":
    sys.exit(main())
