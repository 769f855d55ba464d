"""CPU: the data-gen runner's power profile restated in numpy (nuclear_sim_amd.scenarios.power_profile_rows / power_profile_ramp)
reproduces the reference's own rows bit for bit (tests/golden/power_profile/*.npz, written by tools/make_power_profile_golden.py from
MaintenanceScenarioRunner._generate_power_profile / _set_target_power with a real ConstantHeatSource), for a column of seeds at once
and two runners in a row on one stream; and libnpb.so declares, exports and guards the npb_profile_* entry points (ABI 152).
No compute calls on a device."""
import ctypes
import glob
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nuclear_sim_amd", "libnpb.so")
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "power_profile", "*.npz")))
PROFILE_ENTRY_POINTS = ("npb_profile_seed", "npb_profile_fill", "npb_profile_ramp", "npb_profile_get_state", "npb_profile_set_state")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_the_fixtures_are_there():
    names = {os.path.basename(p)[:-4] for p in GOLDEN}
    assert {"steady_98_0p2", "clipped_104p9_2p0", "floor_20p05_0p1", "noiseless_90_0", "composer_90_2p0"} <= names


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[:-4])
def test_restatement_reproduces_the_reference_bit_for_bit(path):
    from nuclear_sim_amd.scenarios import power_profile_rows
    g = np.load(path)
    seeds = [int(s) for s in g["seeds"]]
    assert {0, 1, 42, 12345, 2 ** 32 - 1} <= set(seeds)
    assert {1, 2, 3, 4, 48, 333} <= {int(T) for T in g["horizons"]}
    base, std = float(g["base_power_percent"]), float(g["noise_std_percent"])
    for T in (int(T) for T in g["horizons"]):
        gens = [np.random.RandomState(s) for s in seeds]
        for run in range(2):          # the second runner draws the next T normals and ramps from a fresh start
            z = np.stack([r.standard_normal(T) for r in gens], axis=1)            # [T, seeds]: every seed's column at once
            target, setpoint = power_profile_rows(z, base, std)
            assert np.array_equal(_bits(target), _bits(g["target_%d" % T][run])), (T, run)
            assert np.array_equal(_bits(setpoint), _bits(g["setpoint_%d" % T][run])), (T, run)
        # exactly 2 T normals were consumed from the global stream
        st = [r.get_state() for r in gens]
        assert [s[2] for s in st] == list(g["state_pos_%d" % T])
        assert [s[3] for s in st] == list(g["state_has_gauss_%d" % T])
        assert np.array_equal(_bits([s[4] for s in st]), _bits(g["state_cached_%d" % T]))
        assert [zlib.crc32(np.ascontiguousarray(s[1], dtype=np.uint32).tobytes()) for s in st] == list(g["state_key_crc32_%d" % T])


def test_the_clip_case_clips():
    """base 104.9 %, std 2.0 % (capped to 0.2), seed 3, 60 steps: 17 raw values are clipped to 105 %"""
    z = np.random.RandomState(3).standard_normal(60)
    assert int(np.sum(104.9 + 0.2 * z > 105.0)) == 17
    from nuclear_sim_amd.scenarios import power_profile_rows
    g = np.load(os.path.join(ROOT, "tests", "golden", "power_profile", "clipped_104p9_2p0.npz"))
    target, setpoint = power_profile_rows(z, 104.9, 2.0)
    j = list(g["seeds"]).index(3)
    assert np.array_equal(_bits(target[:, 0]), _bits(g["target_60"][0, :, j]))
    assert np.array_equal(_bits(setpoint[:, 0]), _bits(g["setpoint_60"][0, :, j]))
    assert target.max() <= 105.0


def test_per_plant_columns_and_the_ramp_alone():
    from nuclear_sim_amd.scenarios import power_profile_ramp, power_profile_rows
    z = np.random.RandomState(9).standard_normal((50, 3))
    base, std = np.array([90.0, 98.0, 104.9]), np.array([2.0, 0.2, 2.0])
    target, setpoint = power_profile_rows(z, base, std)
    for p in range(3):
        t1, s1 = power_profile_rows(z[:, p], base[p], std[p])
        assert np.array_equal(_bits(target[:, p]), _bits(t1[:, 0])) and np.array_equal(_bits(setpoint[:, p]), _bits(s1[:, 0]))
    # the ramp in two calls carries its previous setpoint; a NaN previous setpoint is the first call
    a, prev = power_profile_ramp(target[:20])
    b, _ = power_profile_ramp(target[20:], prev)
    assert np.array_equal(_bits(np.concatenate([a, b])), _bits(setpoint))
    c, _ = power_profile_ramp(target, np.full(3, np.nan))
    assert np.array_equal(_bits(c), _bits(setpoint))
    assert np.all(np.abs(np.diff(setpoint, axis=0)) <= 0.02 + 1e-12) and np.all(np.abs(np.diff(target, axis=0)) <= 0.05 + 1e-12)


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nuclear_sim_amd", "csrc"), "-s"])
    return LIB


def test_header_declares_the_profile_entry_points():
    text = open(os.path.join(ROOT, "include", "npb.h")).read()
    declared = set(re.findall(r"NPB_API[^;]*?\b(npb_\w+)\s*\(", text))
    for s in PROFILE_ENTRY_POINTS:
        assert s in declared, s
    assert int(re.search(r"#define NPB_VERSION (\d+)", text).group(1)) >= 152


def test_library_exports_the_profile_entry_points(built_lib):
    lib = ctypes.CDLL(built_lib)
    for s in PROFILE_ENTRY_POINTS:
        assert hasattr(lib, s), "libnpb.so does not export %s" % s
    assert lib.npb_version() >= 152


def test_binding_declares_them_and_a_null_handle_is_refused(built_lib):
    from nuclear_sim_amd import _lib
    L = _lib.load()
    for s in PROFILE_ENTRY_POINTS:
        assert getattr(L, s).argtypes is not None, s
    assert L.npb_profile_seed(None, None, 1, None, 0, None, 0, None) == -1
    assert L.npb_profile_fill(None, 1, None, None, None, None) == -1
    assert L.npb_profile_ramp(None, 1, None, None, None) == -1
    assert L.npb_profile_get_state(None, None, None, None, None, None, None, None) == -1
    assert L.npb_profile_set_state(None, None, None, None, None, None, 0, None) == -1


def test_a_malformed_power_profile_is_refused_before_any_device_work(built_lib):
    from nuclear_sim_amd.env import BatchedPlantEnv
    with pytest.raises(ValueError):
        BatchedPlantEnv(4, power_profile=dict(seeds=[0, 1, 2, 3]))                       # no steps
    with pytest.raises(ValueError):
        BatchedPlantEnv(4, power_profile=dict(seeds=[0, 1, 2, 3], steps=5, horizon=5))   # an unknown key
    with pytest.raises(ValueError):
        BatchedPlantEnv(4, heat_source="external", power_profile=dict(seeds=[0, 1, 2, 3], steps=5))
