"""Watershed episode statistics without a GPU: the NumPy restatement (tests/ws_stats_ref.py), fed the per-step records of the
engine's NumPy mirror, reproduces bit for bit what the reference's own callbacks computed for the same actions
(tests/golden/watershed/stats_*.npz, written by tests/golden/gen_golden_watershed_stats.py); and summarize()'s reduction."""
import glob
import math
import os

import numpy as np
import pytest

from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd.watershed_stats import DRAINED, METRICS, summarize
from watershed_mirror import WatershedMirror
from ws_stats_ref import WsStatsRef, assert_drains_equal

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "watershed", "stats_*.npz")))


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.int64)


def test_the_five_fixtures_are_there():
    assert [os.path.basename(p) for p in FIXTURES] == ["stats_seq_r0_o0.npz", "stats_seq_r1_o0.npz", "stats_seqcomm_r0_o0.npz",
                                                       "stats_seqcomm_r1_o0.npz", "stats_seqcomm_r1_o1.npz"]


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_restatement_on_the_mirror_equals_the_reference_callbacks(path):
    with np.load(path) as z:
        g = {k: z[k] for k in z.files}
    comm, lr, lo, seed, n, episodes, L = [int(v) for v in g["meta"]]
    m = WatershedMirror(comm, n, seed=seed, local_obs=bool(lo), local_rew=bool(lr))     # env index = fixture row, as the generator's
    ref = WsStatsRef(comm, n)
    t = 0
    for ep in range(episodes):
        m.reset()                                                # the episode key advances with every reset, as the generator's
        ref.reset()
        for k in range(L):
            _, agent, rew, done = m.step(g["actions"][:, t])
            viol, _, running, _, _ = m.info()
            ref.step(rew, done, agent, viol, running)
            t += 1
        assert np.all(done & 2), "the mirror's episode ends where the reference's did"
    assert m.status == 0
    for s in range(n):
        assert len(ref.episodes[s]) == episodes
        for ep, rec in enumerate(ref.episodes[s]):
            assert rec["len"] == g["len"][s, ep] == L
            for key in ("reward", "agent_reward", "total_rews") + METRICS:
                assert np.array_equal(bits(rec[key]), bits(g[key][s, ep])), (s, ep, key, rec[key], g[key][s, ep])
    # ... and the accumulators are those episodes, folded in order
    d = ref.drain()
    assert np.array_equal(d["counts"], np.tile([episodes, 0, episodes * L], (n, 1)))
    for s in range(n):
        total = 0.0
        for ep in range(episodes):
            total = total + float(g["reward"][s, ep])
        assert bits(d["reward_sum"][s]) == bits(total)
        assert np.array_equal(bits(d["last_total_rews"][s]), bits(g["total_rews"][s, -1]))
        for q, name in enumerate(METRICS):
            assert d["metric_counts"][s, q] == episodes
            assert d["metric_min"][s, q] == g[name][s].min() and d["metric_max"][s, q] == g[name][s].max()
    assert_drains_equal(ref.drain(), WsStatsRef(comm, n).drain(), "a drain clears")


def _empty(E):
    d = {name: np.zeros((E,) + shape, dt) for name, dt, shape in DRAINED}
    d["metric_min"][:], d["metric_max"][:] = np.inf, -np.inf
    return d


def test_summarize_means_min_max():
    d = _empty(3)
    d["counts"][:] = [[2, 0, 86], [0, 0, 0], [1, 1, 43]]
    d["reward_sum"][:] = [10.5, 0.0, 0.25]
    d["agent_sums"][0, :4] = [1.0, 2.0, 3.0, 4.5]
    d["agent_sums"][2, :4] = [0.25, 0.0, 0.0, 0.0]
    d["metric_sums"][:] = [[0.5, 2.0, 100.0], [0, 0, 0], [0.25, 1.0, -20.0]]
    d["metric_counts"][:] = [[2, 2, 2], [0, 0, 0], [1, 1, 1]]
    d["metric_min"][0], d["metric_max"][0] = [0.125, 0.75, 40.0], [0.375, 1.25, 60.0]
    d["metric_min"][2], d["metric_max"][2] = [0.25, 1.0, -20.0], [0.25, 1.0, -20.0]
    s = summarize(d, _capi.SSD_WS_SEQ)
    assert s["episodes"] == 3 and s["truncated"] == 1
    assert s["episode_len_mean"] == 129 / 3 and s["episode_reward_mean"] == (10.5 + 0.0 + 0.25) / 3
    assert s["policy_reward_mean"] == {"agent-0": 1.25 / 3, "agent-1": 2.0 / 3, "agent-2": 1.0, "agent-3": 1.5}
    c = s["custom_metrics"]
    assert c["violations_mean"] == 0.75 / 3 and c["violations_min"] == 0.125 and c["violations_max"] == 0.375
    assert c["Equality_mean"] == 1.0 and c["Equality_min"] == 0.75 and c["Equality_max"] == 1.25
    assert c["Utility_mean"] == 80.0 / 3 and c["Utility_min"] == -20.0 and c["Utility_max"] == 60.0
    assert sorted(summarize(d, _capi.SSD_WS_SEQ_COMM)["policy_reward_mean"]) == ["agent-%d" % i for i in range(8)]


def test_summarize_float_sums_go_env_after_env_from_zero():
    d = _empty(3)
    d["counts"][:, 0] = 1
    d["reward_sum"][:] = [1e16, 1.0, -1e16]                      # (1e16 + 1) - 1e16 = 0 in float64; any other order gives 1
    assert summarize(d, _capi.SSD_WS_SEQ)["episode_reward_mean"] == 0.0


def test_summarize_over_nothing_is_nan():
    s = summarize(_empty(4), _capi.SSD_WS_SEQ)
    assert s["episodes"] == 0 and s["truncated"] == 0
    assert math.isnan(s["episode_len_mean"]) and math.isnan(s["episode_reward_mean"])
    assert all(math.isnan(v) for v in s["policy_reward_mean"].values())
    assert len(s["custom_metrics"]) == 9 and all(math.isnan(v) for v in s["custom_metrics"].values())
    # an episode whose metrics were all non-finite counts as an episode and in no metric
    d = _empty(1)
    d["counts"][0] = [1, 0, 43]
    s = summarize(d, _capi.SSD_WS_SEQ)
    assert s["episode_len_mean"] == 43.0 and all(math.isnan(v) for v in s["custom_metrics"].values())


def test_a_truncated_episode_counts_only_in_truncated():
    E = 2
    ref = WsStatsRef(0, E)
    ref.reset()
    zeros6, zeros4 = np.zeros((E, 6), np.uint8), np.zeros((E, 4))
    for k in range(5):
        ref.step(np.full(E, 1.5), np.zeros(E, np.uint8), np.full(E, k % 4, np.int8), zeros6, zeros4)
    ref.reset(mask=[True, False])                                 # env 0 is cut short; env 1 goes on and finishes
    ref.reset(mask=[True, False])                                 # ... a second reset of a stepless episode truncates nothing
    ref.step(np.full(E, 2.0), np.array([0, 2], np.uint8), np.full(E, 3, np.int8), zeros6, np.ones((E, 4)))
    ref.step(np.full(E, 8.0), np.zeros(E, np.uint8), np.zeros(E, np.int8), zeros6, zeros4)   # env 1 is closed: not counted
    d = ref.drain()
    assert d["counts"].tolist() == [[0, 1, 0], [1, 0, 6]]
    assert d["reward_sum"].tolist() == [0.0, 9.5] and d["last_len"].tolist() == [0, 6]
    s = summarize(d, 0)
    assert s["episodes"] == 1 and s["truncated"] == 1 and s["episode_len_mean"] == 6.0 and s["episode_reward_mean"] == 9.5
    assert s["custom_metrics"]["Utility_mean"] == 8.0 and s["custom_metrics"]["Equality_mean"] == 1.0
    assert s["custom_metrics"]["violations_mean"] == 0.0


def test_the_entry_points_are_declared():
    assert _capi.WS_STATS_SYMBOLS == ("ssd_ws_stats_create", "ssd_ws_stats_destroy", "ssd_ws_stats_attach", "ssd_ws_stats_discard",
                                      "ssd_ws_stats_drain", "ssd_ws_stats_last_error")
    L = _capi.lib()
    for name in _capi.WS_STATS_SYMBOLS:
        assert name in _capi.SYMBOLS and hasattr(L, name)
    import ctypes as C
    h = C.c_void_p()
    assert L.ssd_ws_stats_create(2, 4, 0, C.byref(h)) == _capi.SSD_E_INVALID and b"variant" in L.ssd_ws_stats_last_error(None)
    assert L.ssd_ws_stats_create(0, 0, 0, C.byref(h)) == _capi.SSD_E_INVALID and b"num_envs" in L.ssd_ws_stats_last_error(None)
