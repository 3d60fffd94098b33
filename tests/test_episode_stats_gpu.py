"""The device fold of the episode statistics (csrc/ssd_stats.hip) against the sequential restatement (episode_stats_ref.py),
bit for bit: synthetic rings, the adapter's tracking, the rollout calls' stats= argument, truncation, argument checks."""
import numpy as np
import pytest
import torch

from episode_stats_ref import RefStats, same, summary
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd.engine import VecEngine
from sequential_social_dilemma_games_amd.episode_stats import EpisodeStats
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _rew(rng, shape):
    # apples, FIRE costs, single and multiple hits, and a zero-sum tail
    return rng.choice([1, 0, 0, -1, -50, -49, -51, -100, -101, -150], size=shape,
                      p=[.25, .3, .1, .1, .08, .05, .04, .04, .02, .02]).astype(np.int32)


def _check_drain(st, ref):
    got, want = st.drain(), ref.drain()
    assert same(got, want), {k: (got[k], want[k]) for k in got if not same(got[k], want[k])}
    return got


@pytest.mark.parametrize("N", [1, 5, 10, 64])
def test_synthetic_rings_fold_to_the_restatement(N):
    rng = np.random.default_rng(100 + N)
    E = 37 if N < 64 else 3
    ref = RefStats(E, N)
    st = EpisodeStats(E, N)
    # (ring, step0, n_steps, reset_every, done probability, chunk)
    calls = [(7, 3, 7, 0, 0.2, 0), (5, 0, 1, 0, 0.5, 0), (13, 11, 9, 4, 0.0, 3), (2000, 0, 2000, 0, 0.01, 0),
             (300, 17, 250, 0, 0.003, 1), (31, 31, 30, 31, 0.05, 64), (64, 5, 64, 0, 0.0, 7), (9, 2, 9, 0, 1.0, 0)]
    for ring, step0, n, re, p, chunk in calls:
        rew = _rew(rng, (ring, E, N))
        if rng.random() < 0.3:
            rew[:, :2] = 0                                       # envs with C = 0 and no positive reward
        done = (rng.random((ring, E, 1)) < p).astype(np.uint8).repeat(N, axis=2)
        use_done = p > 0
        st.set_chunk(chunk)
        st.fold(torch.from_numpy(rew).to(DEV), torch.from_numpy(done).to(DEV) if use_done else None, step0=step0, n_steps=n,
                reset_every=re)
        ref.fold(rew, done if use_done else None, step0=step0, n_steps=n, reset_every=re)
        if rng.random() < 0.4:
            d = _check_drain(st, ref)
    d = _check_drain(st, ref)
    assert d is not None


def test_chunking_never_changes_a_result():
    rng = np.random.default_rng(7)
    E, N, n = 50, 5, 1000
    rew = torch.from_numpy(_rew(rng, (n, E, N))).to(DEV)
    done = torch.from_numpy((rng.random((n, E, 1)) < 0.02).astype(np.uint8).repeat(N, axis=2)).to(DEV)
    outs = []
    for chunk in (0, 1, 2, 5, 64, 333, 1000):
        st = EpisodeStats(E, N)
        st.set_chunk(chunk)
        st.fold(rew, done, step0=0, n_steps=600)
        st.fold(rew, done, step0=600, n_steps=400)
        outs.append(st.drain())
    ref = RefStats(E, N)
    ref.fold(rew.cpu().numpy(), done.cpu().numpy(), 0, 600)
    ref.fold(rew.cpu().numpy(), done.cpu().numpy(), 600, 400)
    want = ref.drain()
    for o in outs:
        assert same(o, want)


def test_vector_env_tracking_harvest():
    E, N, steps = 4096, 5, 350
    plain = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=100, seed=3)
    tracked = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=100, seed=3, track_episodes=True)
    o1, o2 = plain.reset(), tracked.reset()
    assert torch.equal(o1, o2)
    rews, dones = [], []
    for _ in range(steps):
        a, r1, d1 = plain.step_random()
        b, r2, d2 = tracked.step_random()
        assert torch.equal(a, b) and torch.equal(r1, r2) and torch.equal(d1, d2)
        rews.append(r1.clone())
        dones.append(d1.clone())
    ref = RefStats(E, N)
    ref.fold(torch.stack(rews).cpu().numpy(), torch.stack(dones).cpu().numpy())
    want = ref.drain()
    got = tracked.episode_stats().drain(keep=True)
    assert same(got, want)
    assert int(got["counts"][:, 0].sum()) == 3 * E             # horizon 100: three episodes per env in 350 steps
    assert same(tracked.summary(), summary(want, N))
    assert not tracked.episode_stats().drain()["counts"].any()  # summary() drained


def test_vector_env_summary_and_try_reset_truncate():
    E, N = 64, 5
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=30, seed=9, track_episodes=True, track_ring=16)
    env.reset()
    rews, dones = [], []
    for _ in range(45):
        _, r, d = env.step_random()
        rews.append(r.clone())
        dones.append(d.clone())
    ref = RefStats(E, N)
    ref.fold(torch.stack(rews).cpu().numpy(), torch.stack(dones).cpu().numpy())
    env.try_reset(3)                                             # env 3 is 15 steps into its second episode: truncated
    ref.discard(np.arange(E) == 3)
    s = env.summary()
    assert same(s, summary(ref.drain(), N))
    assert s["episodes"] == E and s["truncated"] == 1
    env.reset()                                                  # every env with an open episode (all but env 3) is cut
    ref.discard()
    d = env.episode_stats().drain()
    assert same(d, ref.drain()) and int(d["counts"][:, 1].sum()) == E - 1


@pytest.mark.parametrize("fused", [True, False, "auto"])
def test_rollout_random_with_stats(fused):
    E, N = 1000, 5
    drains = []
    for split in ((300,), (150, 150), (100, 100, 100)):
        eng = VecEngine(K.GAME_HARVEST, None, num_envs=E, num_agents=N, seed=21)
        eng.reset()
        st = EpisodeStats(E, N)
        rew = torch.zeros((300, E, N), dtype=torch.int32, device=DEV)     # (the outputs share one ring: no obs here)
        step0 = 0
        for n in split:
            eng.rollout_random(n, None, rew, None, reset_every=100, step0=step0, fused=fused, stats=st)
            step0 += n
        drains.append((st.drain(), rew.cpu().numpy()))
    ref = RefStats(E, N)
    ref.fold(drains[0][1], None, step0=0, n_steps=300, reset_every=100)
    want = ref.drain()
    for d, r in drains:
        assert np.array_equal(r, drains[0][1])
        assert same(d, want)
    assert int(want["counts"][:, 0].sum()) == 3 * E


@pytest.mark.parametrize("game,amap_name,N", [(K.GAME_CLEANUP, None, 5), (K.GAME_CLEANUP, "g25_cleanup_48x36_n10_v7", 10),
                                              (K.GAME_HARVEST, None, 1), (K.GAME_HARVEST, None, 2)])
def test_rollout_actions_with_stats(game, amap_name, N):
    import golden_util as G
    amap = G.load(amap_name).map if amap_name else None
    E, n = 300, 240
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, seed=5)
    eng.reset()
    st = EpisodeStats(E, N)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    acts = torch.randint(-1, eng.num_actions, (n, E, N), dtype=torch.int32, device=DEV, generator=gen)
    rew = torch.zeros((n, E, N), dtype=torch.int32, device=DEV)
    eng.rollout_actions(acts, 100, None, rew, None, reset_every=70, step0=0, stats=st)
    eng.rollout_actions(acts, 140, None, rew, None, reset_every=70, step0=100, stats=st)
    ref = RefStats(E, N)
    r = rew.cpu().numpy()
    ref.fold(r, None, 0, 100, 70)
    ref.fold(r, None, 100, 140, 70)
    want = ref.drain()
    assert same(st.drain(), want)
    assert int(want["counts"][:, 0].sum()) == 3 * E


def test_malformed_calls_raise_before_any_launch():
    E, N = 8, 5
    eng = VecEngine(K.GAME_HARVEST, None, num_envs=E, num_agents=N, seed=1)
    eng.reset()
    st = EpisodeStats(E, N)
    obs = torch.empty((4, E, N, 15, 15, 3), dtype=torch.uint8, device=DEV)
    rew = torch.zeros((4, E, N), dtype=torch.int32, device=DEV)
    before = eng.get_state()["t"].copy()
    with pytest.raises(ValueError):
        eng.rollout_random(5, obs, rew, stats=st)               # ring 4 < 5 steps
    with pytest.raises(ValueError):
        eng.rollout_random(2, obs, None, stats=st)              # stats without rew
    with pytest.raises(ValueError):
        eng.rollout_random(2, obs, rew, stats=EpisodeStats(E, 4))
    acts = torch.zeros((4, E, N), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        eng.rollout_actions(acts, 5, obs, rew, stats=st)
    assert np.array_equal(eng.get_state()["t"], before)         # nothing stepped
    for bad in (rew.to(torch.int64), rew.cpu(), rew[:, :, :4].contiguous(), rew.transpose(0, 1), rew[0]):
        with pytest.raises(ValueError):
            st.fold(bad)
    with pytest.raises(ValueError):
        st.fold(rew, torch.zeros((4, E, N), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        st.fold(rew, n_steps=5)
    with pytest.raises(ValueError):
        st.discard(torch.zeros(E + 1, dtype=torch.uint8, device=DEV))
    d = st.drain()
    assert not d["counts"].any() and not d["metric_counts"].any()
