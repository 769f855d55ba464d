"""CPU: what bench.py --dump-outputs keeps of a step's outputs (bench.last_step_outputs), on host tensors shaped like the env's."""
import importlib.util
import os

import numpy as np
import torch


def _bench():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    return bench


def _step_outputs(n):
    g = torch.Generator().manual_seed(0)
    obs = torch.randn((n, 22), dtype=torch.float64, generator=g)
    reward = torch.randn(n, dtype=torch.float64, generator=g)
    done = (torch.rand(n, generator=g) < 0.1).to(torch.uint8)
    info = {"electrical_power": torch.randn(n, dtype=torch.float64, generator=g),
            "trip_flags": torch.randint(0, 1 << 30, (n,), dtype=torch.int32, generator=g), "scram_activated": done}
    return obs, reward, done, info


def _check_rows(out, obs, reward, done, info, lo):
    rows = out["plant_index"].astype(np.int64) - lo
    assert np.array_equal(out["obs"], obs.numpy()[rows]) and np.array_equal(out["reward"], reward.numpy()[rows])
    assert np.array_equal(out["done"], done.numpy()[rows].astype(np.float64))
    for k, v in info.items():
        assert np.array_equal(out["info_" + k], v.numpy()[rows].astype(np.float64)), k      # int32 flags are exact in float64
    return rows


def test_dump_keeps_every_plant_when_they_fit():
    bench = _bench()
    obs, reward, done, info = _step_outputs(1000)
    out = bench.last_step_outputs(obs, reward, done, info, lo=4096)
    assert set(out) == {"plant_index", "obs", "reward", "done", "info_electrical_power", "info_trip_flags", "info_scram_activated"}
    assert all(a.dtype == np.float64 for a in out.values())
    assert np.array_equal(_check_rows(out, obs, reward, done, info, 4096), np.arange(1000))


def test_dump_samples_the_same_plants_within_its_bound():
    bench = _bench()
    bench.DUMP_BYTES = 100_000
    obs, reward, done, info = _step_outputs(5000)
    out = bench.last_step_outputs(obs, reward, done, info, lo=0)
    assert sum(a.nbytes + 128 for a in out.values()) <= bench.DUMP_BYTES
    rows = _check_rows(out, obs, reward, done, info, 0)
    assert 0 < len(rows) < 5000 and np.all(np.diff(rows) > 0)
    again = bench.last_step_outputs(obs, reward, done, info, lo=0)
    assert all(np.array_equal(out[k], again[k]) for k in out)

