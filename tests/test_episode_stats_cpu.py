"""CPU checks of the episode statistics: the restatement on hand-computed episodes, the reward decode that the statistics
rest on (r = a - f - 50h) over the reference fixtures and over oracle rollouts, and the C ABI's argument checks."""
import ctypes as C

import numpy as np
import pytest

import golden_util as G
from episode_stats_ref import RefStats, metrics, same, summary
from oracle import pyoracle
from sequential_social_dilemma_games_amd import _capi, config
from sequential_social_dilemma_games_amd.episode_stats import summarize

FIRE = 7                                                         # Harvest and Cleanup alike (agent.py action maps)


def test_hand_computed_episode():
    # N = 2, T = 4.  agent 0: apple at t=1 and t=3, hit twice at t=4 (r = -100);  agent 1: fires at t=2 (-1), apple at t=4
    rew = np.array([[[1, 0]], [[0, -1]], [[1, 0]], [[-100, 1]]], np.int32)
    ref = RefStats(1, 2)
    ref.fold(rew, reset_every=4)
    d = ref.drain()
    assert d["counts"].tolist() == [[1, 0, 4, -98]]
    assert d["agent_sums"].tolist() == [[[-98, 0], [2, 0], [1, 0]]]
    U, Eq, S, P = d["last_metrics"][0]
    assert U == -98 / 4
    assert Eq == 1.0 - 196 / (2 * 2 * -98)                       # negative C: the formula's value, meaningless
    assert S == ((1 + 3) / 2 + 4 / 1) / 2
    assert P == (2 * 4 - 1) / 4
    assert d["metric_counts"].tolist() == [[1, 1, 1, 1]]


def test_zero_collective_return_and_no_positive_reward():
    U, Eq, S, P = metrics([0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], 5)
    assert U == 0.0 and np.isnan(Eq) and np.isnan(S) and P == 3.0
    U, Eq, S, P = metrics([1, -1], [1, 0], [1, 0], [0, 0], 1)  # C = 0, G > 0: -inf
    assert Eq == -np.inf and S == 1.0
    # non-finite values are skipped in the sums and counts, kept in the last record
    ref = RefStats(1, 3)
    ref.fold(np.zeros((5, 1, 3), np.int32), reset_every=5)
    d = ref.drain()
    assert d["metric_counts"].tolist() == [[1, 0, 0, 1]] and np.isnan(d["last_metrics"][0, 1])
    s = summary(d, 3)
    assert np.isnan(s["equality"]) and np.isnan(s["sustainability"]) and s["efficiency"] == 0.0 and s["episodes"] == 1


def test_one_step_episodes_and_truncation():
    ref = RefStats(2, 1)
    rew = np.array([[[1], [0]], [[-50], [1]], [[0], [0]]], np.int32)
    done = np.zeros((3, 2, 1), np.uint8)
    done[:, 0, 0] = 1                                            # env 0: every step ends an episode
    ref.fold(rew, done)
    d = ref.drain(keep=True)
    assert d["counts"][:, 0].tolist() == [3, 0] and d["counts"][:, 2].tolist() == [3, 0]
    assert d["agent_sums"][0, 1, 0] == 1 and d["agent_sums"][0, 2, 0] == 1           # one hit, one tagged step
    assert d["last_len"].tolist() == [1, 0]
    ref.discard(np.array([0, 1], np.uint8))                     # env 1 had 3 open steps
    ref.fold(rew, None, step0=3, reset_every=3)                 # 3 % 3 == 0: everything open is cut first (nothing is)
    d = ref.drain()
    assert d["counts"][:, 1].tolist() == [0, 1] and d["counts"][:, 0].tolist() == [4, 1]


def test_summarize_matches_the_restatement():
    rng = np.random.default_rng(5)
    E, N = 7, 3
    ref = RefStats(E, N)
    for step0 in (0, 13, 40):
        rew = rng.choice([1, 0, -1, -50, -51, -100], size=(20, E, N), p=[.3, .3, .1, .15, .1, .05]).astype(np.int32)
        done = (rng.random((20, E, N)) < 0.1).astype(np.uint8)
        ref.fold(rew, done, step0=step0, n_steps=17, reset_every=9)
    d = ref.drain()
    assert same(summarize(d, N), summary(d, N))


def _decode_check(rew, act):
    r = rew.astype(np.int64)
    h = (1 - r) // 50
    f = (act == FIRE).astype(np.int64)
    a = r + 50 * h + f
    assert np.all((a == 0) | (a == 1)), "r = a - f - 50h does not hold"
    assert np.array_equal(r > 0, (a == 1) & (f == 0) & (h == 0))
    return int((h > 0).sum()), int((h > 1).sum()), r.size


def test_reward_decode_on_every_fixture():
    hits = multi = n = 0
    for g in G.groups():
        if not g.steps:
            continue
        a, b, c = _decode_check(g.steps["rew"], g.steps["act"])
        hits, multi, n = hits + a, multi + b, n + c
    assert n > 30000 and hits > 1000 and multi > 10, (n, hits, multi)


def test_reward_decode_on_oracle_rollouts_cleanup_48x36():
    g = G.load("g25_cleanup_48x36_n10_v7")
    ora = pyoracle.Oracle(g.game, g.map, 16, 10, config.make_lut(), seed=11)
    ora.reset()
    hits = multi = 0
    for _ in range(300):
        act, _, rew, _ = ora.step_random(want_obs=False)
        a, b, _ = _decode_check(rew, act)
        hits, multi = hits + a, multi + b
    assert hits > 0 and multi > 0, (hits, multi)


def test_stats_create_checks_arguments_and_needs_a_gpu():
    import torch
    L = _capi.lib()
    h = C.c_void_p()
    assert L.ssd_stats_create(4, 0, 0, C.byref(h)) == _capi.SSD_E_INVALID
    assert L.ssd_stats_create(0, 5, 0, C.byref(h)) == _capi.SSD_E_INVALID
    assert L.ssd_stats_create(4, 65, 0, C.byref(h)) == _capi.SSD_E_INVALID
    assert b"num_agents" in L.ssd_stats_last_error(None)
    rc = L.ssd_stats_create(4, 5, 0, C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0
        assert L.ssd_stats_fold(h, C.c_void_p(16), None, 4, 0, 5, 0, 0, None) == _capi.SSD_E_INVALID     # n_steps > ring
        L.ssd_stats_destroy(h)
    else:
        assert rc == _capi.SSD_E_DEVICE
        assert b"no CPU path" in L.ssd_stats_last_error(None)
    assert _capi.SSD_STATS_KEEP == 1


def test_episode_stats_is_exported():
    import sequential_social_dilemma_games_amd as pkg
    from sequential_social_dilemma_games_amd.episode_stats import EpisodeStats
    assert pkg.EpisodeStats is EpisodeStats
    with pytest.raises(_capi.SsdError):
        import torch
        if torch.cuda.is_available():
            raise _capi.SsdError("GPU present")
        EpisodeStats(4, 5)
