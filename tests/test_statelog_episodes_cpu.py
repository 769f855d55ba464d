"""CPU: the state log's history-window columns per (plant, episode) -- statelog._episode_windows over synthetic series: each episode's
rows episode_step >= 1 are windowed on their own when the log holds them from step 1 on without a gap, and everything else is NaN."""
import numpy as np

from nuclear_sim_amd import statelog


def test_each_episode_is_windowed_on_its_own():
    hist = statelog.history_log_columns()
    rms = hist["secondary.ph_control.ph_control_deviation_rms"][1]
    tic = hist["secondary.ph_control.ph_control_time_in_control"][1]
    rng = np.random.default_rng(3)
    ns = 12
    series = rng.uniform(-0.1, 0.1, (ns, 3))
    # plant 0: one episode from step 1; plant 1: restarts on sample 4 (a step-0 row) and runs on; plant 2: joins the log at step 5 of
    # episode 0 (its step 1 is not in the log), restarts on sample 6
    step = np.stack([np.arange(1, ns + 1),
                     np.array([1, 2, 3, 4, 0, 1, 2, 3, 4, 5, 6, 7]),
                     np.array([5, 6, 7, 8, 9, 10, 0, 1, 2, 3, 4, 5])], axis=1)
    episode = np.stack([np.zeros(ns, dtype=np.int64),
                        np.array([0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1]),
                        np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1])], axis=1)
    for fn in (rms, tic):
        got = statelog._episode_windows(fn, [series], episode, step)
        assert np.array_equal(got[:, 0], fn(series[:, 0:1])[:, 0])
        assert np.array_equal(got[:4, 1], fn(series[:4, 1:2])[:, 0]) and np.isnan(got[4, 1])
        assert np.array_equal(got[5:, 1], fn(series[5:, 1:2])[:, 0])
        assert np.isnan(got[:7, 2]).all() and np.array_equal(got[7:, 2], fn(series[7:, 2:3])[:, 0])
    # a window that really depends on where the episode starts: the share of steps inside the deadband restarts at the restart
    inside = np.where(np.arange(ns) < 5, 0.01, 0.2)[:, None] * np.ones((1, 3))
    got = statelog._episode_windows(tic, [inside], episode, step)
    assert got[3, 1] == 100.0 and got[5, 1] == 0.0 and abs(got[-1, 0] - 100.0 * 5 / 12) < 1e-12


def test_the_npsh_trend_takes_four_sources_and_a_gap_gives_nan():
    trend = statelog.history_log_columns()["secondary.feedwater_SECONDARY-COMP-001-FW.protection_npsh_trend"][1]
    rng = np.random.default_rng(4)
    ns = 8
    src = [rng.uniform(5.0, 20.0, (ns, 2)) for _ in range(4)]
    step = np.stack([np.array([1, 2, 3, 0, 1, 2, 3, 4]), np.array([1, 2, 4, 5, 6, 7, 8, 9])], axis=1)       # plant 1: step 3 is missing
    episode = np.stack([np.array([0, 0, 0, 1, 1, 1, 1, 1]), np.zeros(ns, dtype=np.int64)], axis=1)
    got = statelog._episode_windows(trend, src, episode, step)
    assert np.array_equal(got[:3, 0], trend(*[s[:3, 0:1] for s in src])[:, 0]) and np.isnan(got[3, 0])
    assert np.array_equal(got[4:, 0], trend(*[s[4:, 0:1] for s in src])[:, 0])
    assert np.isnan(got[:, 1]).all()
