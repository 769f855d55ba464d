"""When does a maintenance action first fire in each of M scenarios?  M scenario seeds streamed through fewer lanes.

    python tools/banked_trigger_sweep.py oil_top_off --seeds 200 264 --lanes 16 --hours 2.5 --dt 5 --out triggers.parquet

The command-line face of nuclear_sim_amd.timing.banked_trigger_times: one env of `--lanes` plants whose start bank holds the scenarios
of seeds [first, last), autoreset with the episode limit hours * 60 / dt, episode streams, a one-key work-order summary and episode
records that carry each finished episode's summary rows.  Writes one row per seed -- seed, first_created_hours, first_completed_hours
(empty = never), n_created, n_completed, length, terminated -- as Parquet, or CSV for a path ending in .csv, and prints a one-line
JSON summary.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("action", help="a feedwater maintenance action, e.g. oil_top_off")
    ap.add_argument("--seeds", type=int, nargs=2, metavar=("FIRST", "LAST"), required=True, help="scenario seeds FIRST .. LAST - 1")
    ap.add_argument("--lanes", type=int, required=True, help="plants the scenarios are streamed through (<= number of seeds)")
    ap.add_argument("--hours", type=float, required=True, help="length of every scenario's run")
    ap.add_argument("--dt", type=float, default=1.0, help="minutes per step")
    ap.add_argument("--unit", type=int, default=None, help="restrict to one pump (0..3)")
    ap.add_argument("--power-setpoint", type=float, default=90.0)
    ap.add_argument("--storage", choices=["f64", "f32"], default="f64")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", required=True, help="the table: .csv = CSV, anything else Parquet")
    a = ap.parse_args()
    from nuclear_sim_amd import maintlog
    from nuclear_sim_amd.timing import banked_trigger_times
    seeds = list(range(a.seeds[0], a.seeds[1]))
    r = banked_trigger_times(a.action, seeds, a.hours, a.lanes, dt=a.dt, unit=a.unit, power_setpoint=a.power_setpoint, device=a.device,
                             storage=a.storage)
    cols = {"seed": np.asarray(seeds, dtype=np.int64)}
    cols.update({k: r[k] for k in ("first_created_hours", "first_completed_hours", "n_created", "n_completed", "length", "terminated")})
    maintlog.write(cols, a.out)
    fired = np.isfinite(r["first_created_hours"])
    print(json.dumps({"action": a.action, "seeds": len(seeds), "lanes": a.lanes, "steps": r["steps"], "fired": int(fired.sum()),
                      "median_first_created_hours": float(np.median(r["first_created_hours"][fired])) if fired.any() else None,
                      "dropped": r["dropped"], "out": a.out}))


if __name__ == "__main__":
    main()
